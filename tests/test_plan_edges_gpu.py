"""The compiled replay list of a launch plan (csrc/plan_edges.h: duplicate records aliased, records folded into their
producing launch, dominated / clustered waits dropped) orders the device work exactly as the recorded list does:
  * a plan of library kernels handing fp32 buffers from the main stream to two side streams gives, bit for bit, what
    the same kernels give on one stream and what the verbatim replay (edge mode 0) gives;
  * the small cond-UNet trainer (side streams, context branch, chunked optimizer) reaches bitwise the same state after
    three replays in edge mode 0 and in edge mode 1, and sync_optimizer() still waits for the optimizer (the caller's
    events are recorded on every replay);
  * the pass finds something of every kind in the recorded cond-UNet step."""
import ctypes

import pytest
import torch

from oracle import sd_oracle as O
from tests.golden.configs import SMALL_COND

pytestmark = pytest.mark.gpu


@pytest.fixture
def edges():
    """Sets the process-wide edge mode; back to the default (1) afterwards."""
    from sdmi import _lib
    L = _lib.lib()

    def set_mode(m):
        _lib.check(L.sdmi_plan_set_edges(m), "sdmi_plan_set_edges")
    yield set_mode
    set_mode(1)


N_HANDOFF = 72
ELEMS = 1 << 18  # 1 MB fp32 per buffer


def _combine(c, u, scale, out, stream):
    """out = u + scale * (c - u) (sdmi_cfg_combine: sub, mul, add rounded separately) on `stream`."""
    from sdmi import _lib
    _lib.check(_lib.lib().sdmi_cfg_combine(c.data_ptr(), u.data_ptr(), c.numel(), scale, out.data_ptr(),
                                           ctypes.c_void_p(stream.cuda_stream)), "sdmi_cfg_combine")


def _handoffs(x, bufs, acc, main, sides, final):
    """The main stream produces buffer i from buffer i - 1 and x; a side stream folds it into its accumulator; the main
    stream joins both at the end. sides = (main, main): the same kernels on one stream, no edges."""
    from sdmi import plan as P
    one = sides[0] is main
    for i in range(N_HANDOFF):
        _combine(x, bufs[i - 1] if i else x, 0.25 + 0.01 * i, bufs[i], main)
        if i % 4 == 3:  # both sides consume it: two private edges off the main stream, back to back (duplicate record)
            targets = [0, 1]
        else:
            targets = [i % 2]
        if not one:
            if i % 3 == 1:  # a caller's event, waited for twice (doubled wait)
                ev = torch.cuda.Event()
                P.record_event(ev, main)
                for k in targets:
                    P.wait_event(sides[k], ev)
                    P.wait_event(sides[k], ev)
            else:
                for k in targets:
                    P.wait_stream(sides[k], main)
        for k in targets:
            _combine(bufs[i], acc[k], 0.5, acc[k], sides[k])
    if not one:
        for s in sides:
            P.wait_stream(main, s)
            P.wait_stream(main, s)
    _combine(acc[0], acc[1], 0.5, final, main)


def test_handoff_plan_matches_one_stream_and_verbatim_replay(edges):
    from sdmi.plan import StepPlan
    dev = torch.device("cuda", 0)
    main = torch.cuda.current_stream(dev)
    sides = (torch.cuda.Stream(dev), torch.cuda.Stream(dev))
    g = torch.Generator().manual_seed(11)
    xs = [torch.randn(ELEMS, generator=g).to(dev) for _ in range(4)]

    def fresh():
        return (torch.empty(ELEMS, device=dev), [torch.empty(ELEMS, device=dev) for _ in range(N_HANDOFF)],
                [torch.zeros(ELEMS, device=dev) for _ in range(2)], torch.empty(ELEMS, device=dev))

    # the same kernels on one stream: four rounds (the recording run and three replays), accumulators carried along
    x, bufs, acc, final = fresh()
    want = []
    for r in range(4):
        x.copy_(xs[r])
        _handoffs(x, bufs, acc, main, (main, main), final)
        want.append((final.clone(), acc[0].clone(), acc[1].clone()))
    torch.cuda.synchronize()

    got = {}
    for mode in (1, 0):
        x, bufs, acc, final = fresh()
        torch.cuda.synchronize()
        x.copy_(xs[0])
        plan = StepPlan(lambda: _handoffs(x, bufs, acc, main, sides, final))
        info = plan.edge_info()
        assert info["aliased"] >= N_HANDOFF // 4 // 2 and info["waits_dropped"] >= N_HANDOFF // 3
        assert info["compiled"] < info["recorded"] == len(plan)
        edges(mode)
        got[mode] = []
        for r in range(1, 4):
            x.copy_(xs[r])
            plan.replay()
            got[mode].append((final.clone(), acc[0].clone(), acc[1].clone()))
        torch.cuda.synchronize()
        for r in range(1, 4):
            for a, b in zip(got[mode][r - 1], want[r]):
                assert torch.equal(a, b), (mode, r)
    for r in range(3):
        for a, b in zip(got[0][r], got[1][r]):
            assert torch.equal(a, b)


def _inputs(step, B=2):
    g = torch.Generator().manual_seed(900 + step)
    x0 = torch.randn(B, 4, 32, 32, generator=g)
    noise = torch.randn(B, 4, 32, 32, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    text = torch.randn(B, 77, 64, generator=g)
    cmap = torch.randint(0, 19, (B, 64, 64), generator=g)
    mask = torch.nn.functional.one_hot(cmap, 19).movedim(-1, 1)[:, 1:].float()
    keep = (torch.rand(B, generator=g) > 0.3).float()
    return [v.cuda() for v in (x0, noise, t, text, mask, keep)]


def _replayed_trainer(mode, edges):
    """A small cond-UNet trainer after the recorded step and three replays in edge mode `mode`."""
    from sdmi.plan import StepPlan
    from sdmi.trainer import DDPMTrainer
    sd = O.deterministic_state(O.unet_param_shapes(SMALL_COND), seed=5)
    tr = DDPMTrainer(SMALL_COND, sd, "cuda", lr=1e-3)
    assert tr.opt_ranges is not None and tr.engine.side is not None and tr.engine.ctx_stream is not None
    bufs = [torch.empty_like(v) for v in _inputs(0)]
    edges(mode)
    plan = None
    for s in range(4):
        for b, v in zip(bufs, _inputs(s)):
            b.copy_(v)
        if s == 0:
            plan = StepPlan(lambda: tr.step(*bufs[:5], mask_keep=bufs[5]))
        else:
            plan.replay()
    return tr, plan


def test_cond_unet_replays_bitwise_equal_in_both_edge_modes(edges):
    from bench import trainer_outputs
    outs = {}
    for mode in (0, 1):
        tr, plan = _replayed_trainer(mode, edges)
        if mode == 1:
            # the optimizer chunks' events are the caller's: recorded on every replay, so the current stream, having
            # waited for them, reads the finished parameters
            tr.sync_optimizer()
            early = tr.store.params.clone()
            torch.cuda.synchronize()
            assert torch.equal(early, tr.store.params)
        outs[mode] = {k: v.clone() for k, v in trainer_outputs(tr).items()}
        torch.cuda.synchronize()
        del plan, tr
    assert set(outs[0]) >= {"state", "params", "grads", "adam_m", "adam_v", "ema"}
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_cond_unet_plan_edge_counters(edges):
    tr, plan = _replayed_trainer(1, edges)
    torch.cuda.synchronize()
    info = plan.edge_info()
    print(info)
    assert info["recorded"] == len(plan)
    assert info["folded"] >= 1 and info["aliased"] >= 1 and info["waits_dropped"] >= 1
    assert info["owned_events"] >= 1
    assert info["compiled"] < info["recorded"]
    assert info["compiled"] == info["recorded"] - info["folded"] - info["aliased"] - info["waits_dropped"]
