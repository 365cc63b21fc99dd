"""The tolerance of the two-forward GPU test (tests/test_autograd_contract_gpu.py, C1) can see the defect it is for.

The mechanism, as a toy: an autograd Function whose backward writes its gradient into ONE buffer kept between calls and
returns a view of it. When two forwards share a graph, the first backward's view waits in autograd's input buffer
(the parameter's `.grad` is still None, so nothing marks the buffer as taken) while the second backward overwrites it:
the accumulated gradient is twice one of the two, and a gradient a caller kept from torch.autograd.grad changes under
their hands. sdmi.module_glue.EngineHolder.grad_buffer had exactly this shape; `storage in use` is its repair.

The GPU test compares the module's gradient of W_A * loss(a) + W_B * loss(b) with the CPU oracle's at the suite's usual
bound (global norm within 5 %, every per-tensor cosine >= 0.99). Here, with the oracle alone, every failure mode --
2 g_a, 2 g_b, g_a alone, g_b alone -- is shown to miss BOTH bounds for every module, so that check cannot pass by
accident. The table is printed."""
import pytest
import torch

from tests import autograd_cases as AC


class _Reuse:
    """How a backward gets its gradient buffer."""

    def __init__(self, guarded):
        self.guarded, self.buf, self.storage, self.allocations = guarded, None, None, 0

    def buffer(self, n):
        free = self.buf is not None and (
            not self.guarded or torch._C._storage_Use_Count(self.storage._cdata) == 2)  # the buffer + `storage`
        if not free:
            self.buf = torch.empty(n)
            self.storage = self.buf.untyped_storage()
            self.allocations += 1
        return self.buf


class _Toy(torch.autograd.Function):
    """F(x, w) = sum(x * w); dF/dw = x, written into the reused buffer and returned as a view of it."""

    @staticmethod
    def forward(ctx, reuse, x, w):
        ctx.reuse, ctx.x = reuse, x
        return (x * w).sum()

    @staticmethod
    def backward(ctx, d):
        buf = ctx.reuse.buffer(ctx.x.numel())
        torch.mul(ctx.x, d, out=buf)
        return None, None, buf[:]


X1, X2 = torch.tensor([1.0, 2.0, 3.0]), torch.tensor([10.0, 20.0, 40.0])


def test_toy_unguarded_reuse_gives_twice_one_gradient():
    r = _Reuse(guarded=False)
    w = torch.ones(3, requires_grad=True)
    (4 * _Toy.apply(r, X1, w) + _Toy.apply(r, X2, w)).backward()
    assert not torch.equal(w.grad, 4 * X1 + X2)
    assert torch.equal(w.grad, 8 * X1) or torch.equal(w.grad, 2 * X2)  # (which one: autograd's node order)
    w.grad = None
    kept, = torch.autograd.grad(_Toy.apply(r, X1, w), [w])
    before = kept.clone()
    _Toy.apply(r, X2, w).backward()
    assert not torch.equal(kept, before) and torch.equal(kept, X2)  # the kept gradient was overwritten


def test_toy_guarded_reuse_is_right_and_still_reuses():
    r = _Reuse(guarded=True)
    w = torch.ones(3, requires_grad=True)
    (4 * _Toy.apply(r, X1, w) + _Toy.apply(r, X2, w)).backward()
    assert torch.equal(w.grad, 4 * X1 + X2)
    w.grad = None
    kept, = torch.autograd.grad(_Toy.apply(r, X1, w), [w])
    before = kept.clone()
    _Toy.apply(r, X2, w).backward()
    assert torch.equal(kept, before) and torch.equal(w.grad, X2)
    _Toy.apply(r, X1, w).backward()  # accumulation without zeroing
    assert torch.equal(w.grad, X2 + X1)
    # the reference loop: `.grad` dropped before each backward -> one buffer for the whole run
    del kept
    w.grad = None
    _Toy.apply(r, X1, w).backward()
    n, ptr = r.allocations, r.buf.data_ptr()
    for _ in range(3):
        w.grad = None
        _Toy.apply(r, X2, w).backward()
        assert torch.equal(w.grad, X2)
    assert r.allocations == n and r.buf.data_ptr() == ptr


@pytest.mark.parametrize("case", AC.ORACLE_CASES, ids=repr)
def test_failure_modes_miss_the_c1_tolerance(case):
    ga, gb = case.oracle("a")[0], case.oracle("b")[0]
    true = AC.combine(ga, gb)
    ratio, worst, _ = AC.against(true, true)
    assert AC.within(ratio, worst)
    row = []
    for mode, g in AC.failure_modes(ga, gb).items():
        ratio, worst, key = AC.against(g, true)
        row.append(f"{mode} {ratio:.2f} / {worst:.2f}")
        assert abs(ratio - 1.0) > AC.NORM_TOL, (mode, ratio)
        assert worst < AC.COS_MIN, (mode, worst, key)
    print(f"\n{case.name}: norm ratio to the true sum / worst per-tensor cosine: " + "; ".join(row))
