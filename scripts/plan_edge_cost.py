"""What one cross-stream edge costs the stream it sits on (sdmi_plan_edge_probe, csrc/plan.hip): a chain of short
dependent kernels on stream A, event-timed on A, against the same chain with an edge at every boundary.
  (a) hipEventRecord on A, flags as torch creates events (hipEventDisableTiming), stream B waiting on each
  (b) the same with hipEventDisableTiming | hipEventDisableSystemFence
  (c) no separate record: the producing kernel launched with hipExtLaunchKernel(stopEvent = ev), both flag sets
  plus the record alone (nothing waiting on it) and with B waiting but running nothing, to tell which half costs;
  (d) hipStreamWaitEvent on A on an event of B that completed long ago
  (e) k = 2, 8, 29 such waits back to back
Per row: the chain's span, and (span - baseline span) / boundaries. Each variant is measured `--rounds` times,
interleaved with the baseline; the table gives every round.
Usage: python scripts/plan_edge_cost.py [--chain 200] [--mb 2] [--reps 5] [--rounds 3]"""
import argparse
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "stablediffusion-pytorch_amd"), REPO]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chain", type=int, default=200)
    ap.add_argument("--mb", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    from sdmi import _lib
    L = _lib.lib()
    nbytes = int(a.mb * (1 << 20))

    def span(variant, nofence=0, k=1):
        us = ctypes.c_float(0)
        _lib.check(L.sdmi_plan_edge_probe(variant, nofence, k, a.chain, nbytes, a.reps, ctypes.byref(us)), "edge probe")
        return us.value

    rows = [("record on A alone (nothing waits), torch flags", 4, 0, 1),
            ("record on A alone (nothing waits), no system fence", 4, 1, 1),
            ("record on A, B waits and runs nothing, torch flags", 5, 0, 1),
            ("(a) record on A, torch flags, B waits", 1, 0, 1),
            ("(b) record on A, no system fence, B waits", 1, 1, 1),
            ("(c) stop event of the launch, torch flags", 2, 0, 1),
            ("(c) stop event of the launch, no system fence", 2, 1, 1),
            ("(d) A waits on a completed event, torch flags", 3, 0, 1),
            ("(d) A waits on a completed event, no system fence", 3, 1, 1),
            ("(e) 2 waits back to back", 3, 0, 2),
            ("(e) 8 waits back to back", 3, 0, 8),
            ("(e) 29 waits back to back", 3, 0, 29)]
    span(0)  # first use: module load, stream creation
    print(f"chain of {a.chain} dependent kernels over {a.mb:g} MB, {a.reps} timed chains per figure, {a.rounds} rounds")
    print(f"{'variant':52s} | " + " | ".join(f"span us  /edge us" for _ in range(a.rounds)))
    base = [span(0) for _ in range(a.rounds)]
    print(f"{'baseline: no edges':52s} | " + " | ".join(f"{b:7.1f}  {b / a.chain:8.2f}" for b in base)
          + "   (/edge: per kernel)")
    for name, variant, nofence, k in rows:
        cells = []
        for r in range(a.rounds):
            b = span(0)
            s = span(variant, nofence, k)
            cells.append(f"{s:7.1f}  {(s - b) / a.chain:8.2f}")
        print(f"{name:52s} | " + " | ".join(cells))


if __name__ == "__main__":
    main()
