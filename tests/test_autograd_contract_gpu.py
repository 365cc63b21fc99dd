"""The autograd contract of the drop-in modules ("The supported autograd surface"): what a caller may do
with a fused module beyond the reference trainer's one forward, one backward, zero_grad(set_to_none=True).

Cases (tests/autograd_cases.py): cond UNet on the single-node and on the staged backward, uncond UNet, DiT, VQVAE,
noise-robust VQVAE and KL autoencoder with a fixed draw -- SMALL_* configs, B = 2 -- and LPIPS where it applies.
`g_a`, `g_b` are the gradients of W_A * loss(a) and W_B * loss(b) from a fresh module each, one forward, one backward.

C1  two forwards in one graph, one backward: `.grad` is bitwise g_a + g_b (one fp32 add; it commutes, so autograd's
    node order does not matter), and agrees with the CPU oracle's gradient of the summed loss at the suite's bound for
    one backward (cosine >= 0.99 per tensor, global norm within 5 %) -- a bound every failure mode misses
    (tests/test_autograd_contract_cpu.py). Precondition, asserted: a repeated single backward reproduces every bit.
C2  a gradient kept from torch.autograd.grad is not touched by a later backward of the same module.
C3  two backwards without zeroing accumulate: bitwise g_a + g_b.
C4  on the reference loop the flat gradient buffer is ONE allocation: same object, same storage, three steps.
C5  an image input that requires grad: the fused forward raises (naming sdmi_leaf_path) before anything is launched,
    with trainable and with frozen parameters; on the leaf path the same call gives the oracle's input gradient.
C6  a frozen subset: trainable parameters get bitwise their unfrozen gradient, frozen ones keep grad None -- also when
    whole segments of the staged backward, or its last one, are frozen.
C7  a backward after a later forward that repacked updated weights raises before launching; without an update in
    between, forward A, forward B, backward A, backward B gives both fresh gradients bitwise. (Updates written through
    `.data` keep the version counters and stay undetected: not tested.)
C8  a second backward through one forward raises (the tape is freed) before launching.
C9  after a staged backward the holder's last_run holds neither the tape nor the prediction nor gradient views.

LPIPS has no parameter gradient and no per-module state a second forward could overwrite (every forward allocates its
own activations, every backward its own outputs; the weights are frozen and packed once), so C1 / C2 / C4 / C6 / C7
do not apply; its image gradients run C1 / C3 in one test, and C8. The raises are host-side checks: no test here
reaches a kernel with a bad argument."""
import gc
import weakref

import pytest
import torch

from tests import autograd_cases as AC

pytestmark = pytest.mark.gpu

CASES = AC.CASES
HOLDER_CASES = [c for c in CASES if c.holder]
_fresh = {}
_aux = {}


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def _single(case, which):
    m = case.build()
    case.loss(m, which).backward()
    torch.cuda.synchronize()
    return m, _grads(m)


def fresh(case, which):
    """g_a / g_b: computed once per case, never written."""
    if (case.name, which) not in _fresh:
        m, g = _single(case, which)
        _fresh[(case.name, which)] = g
        _aux[(case.name, which)] = case.aux(m, which)
    return _fresh[(case.name, which)]


def oracle_sum(case):
    """The CPU oracle's gradient of W_A * loss(a) + W_B * loss(b), at the engine's own discrete choices."""
    fresh(case, "a"), fresh(case, "b")
    oc = AC.BY_NAME["cond"] if case.name == "cond_staged" else case  # same network, same oracle
    return AC.combine(oc.oracle("a", _aux[(case.name, "a")], "engine")[0],
                      oc.oracle("b", _aux[(case.name, "b")], "engine")[0])


def assert_bitwise(got, want, what):
    assert got.keys() == want.keys(), (what, set(got) ^ set(want))
    bad = [k for k in want if not torch.equal(got[k], want[k])]
    assert not bad, f"{what}: {len(bad)} of {len(want)} tensors differ, first {bad[0]}"


def launches(fn):
    """(the exception fn raised or None, the sdmi kernels launched meanwhile) -- the launch recorder of the exact
    tests."""
    from sdmi import _lib
    from tests.attn_matrix import recorded
    box = {}

    def call():
        try:
            fn()
        except Exception as e:  # noqa: BLE001
            box["err"] = e
        return 0
    _, ops = recorded(_lib.lib(), call)
    return box.get("err"), ops


def test_recorder_sees_a_fused_forward():
    """The control of every `ops == []` below."""
    case = AC.BY_NAME["cond"]
    m = case.build()
    with torch.no_grad():
        err, ops = launches(lambda: case.loss(m, "a"))
    assert err is None and len(ops) > 10


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_c1_two_forwards_one_backward(case):
    ga, gb = fresh(case, "a"), fresh(case, "b")
    assert_bitwise(_single(case, "a")[1], ga, "a repeated single backward")
    m = case.build()
    (case.loss(m, "a") + case.loss(m, "b")).backward()
    torch.cuda.synchronize()
    got = _grads(m)
    ratio, worst, key = AC.against(got, oracle_sum(case))
    print(f"\n{case.name}: two forwards, one backward vs the oracle: norm ratio {ratio:.4f}, worst cosine {worst:.5f} "
          f"({key})")
    for mode, g in AC.failure_modes(ga, gb).items():
        if all(torch.equal(got[k], g[k]) for k in g):
            print(f"{case.name}: .grad is bitwise {mode}")
    assert_bitwise(got, AC.combine(ga, gb), "two forwards, one backward vs g_a + g_b")
    assert AC.within(ratio, worst), (ratio, worst, key)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_c2_kept_autograd_grad_survives_a_later_backward(case):
    ga, gb = fresh(case, "a"), fresh(case, "b")
    m = case.build()
    names = [k for k, _ in m.named_parameters()]
    kept = torch.autograd.grad(case.loss(m, "a"), list(m.parameters()))
    clone = [g.clone() for g in kept]
    assert all(p.grad is None for p in m.parameters())
    case.loss(m, "b").backward()
    torch.cuda.synchronize()
    for mode, g in AC.failure_modes(ga, gb).items():
        if mode != "g_a" and all(torch.equal(t, g[k]) for k, t in zip(names, kept)):
            print(f"\n{case.name}: the kept gradient is now bitwise {mode}")
    assert_bitwise(dict(zip(names, kept)), dict(zip(names, clone)), "the kept gradient after a later backward")
    assert_bitwise(dict(zip(names, clone)), ga, "torch.autograd.grad vs g_a")
    assert_bitwise(_grads(m), gb, ".grad after the later backward vs g_b")


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_c3_two_backwards_accumulate(case):
    ga, gb = fresh(case, "a"), fresh(case, "b")
    m = case.build()
    case.loss(m, "a").backward()
    case.loss(m, "b").backward()
    torch.cuda.synchronize()
    assert_bitwise(_grads(m), AC.combine(ga, gb), "two backwards without zeroing vs g_a + g_b")


@pytest.mark.parametrize("case", HOLDER_CASES, ids=repr)
def test_c4_reference_loop_reuses_one_buffer(case):
    m = case.build()
    opt = torch.optim.SGD(m.parameters(), lr=1e-4)
    seen = []
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        case.loss(m, "ab"[step % 2]).backward()
        buf = m._sdmi._gflat
        seen.append((buf, buf.untyped_storage().data_ptr()))
        opt.step()
    torch.cuda.synchronize()
    assert all(b is seen[0][0] and p == seen[0][1] for b, p in seen), [p for _, p in seen]


@pytest.mark.parametrize("frozen", [False, True], ids=["trainable", "frozen"])
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_c5_input_that_requires_grad(case, frozen):
    m = case.build()
    if frozen:
        m.requires_grad_(False)
    x = case.batch("a")["x"].cuda().requires_grad_(True)
    err, ops = launches(lambda: case.loss(m, "a", x=x))
    assert isinstance(err, RuntimeError), repr(err)
    assert "no input gradient" in str(err) and "sdmi_leaf_path = True" in str(err), str(err)
    assert ops == [], ops[:3]
    m.sdmi_leaf_path = True
    aux = case.aux(m, "a")
    case.loss(m, "a", x=x).backward()
    torch.cuda.synchronize()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    assert all((p.grad is None) == frozen for p in m.parameters())
    oc = AC.BY_NAME["cond"] if case.name == "cond_staged" else case
    want = oc.oracle("a", aux, "leaf" if aux is not None else "engine")[1]
    c = AC.cos(x.grad, want)
    r = x.grad.double().norm().item() / want.double().norm().item()
    print(f"\n{case.name}: leaf-path input gradient vs the oracle: cosine {c:.6f}, norm ratio {r:.4f}")
    assert c >= AC.LEAF_COS_MIN, c


@pytest.mark.parametrize("rule", ["half", "tail"])
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_c6_frozen_subset(case, rule):
    full = fresh(case, "a")
    m = case.build()
    frozen = {k for k, _ in m.named_parameters() if case.frozen(k, rule)}
    assert 0 < len(frozen) < len(full)
    for k, p in m.named_parameters():
        p.requires_grad_(k not in frozen)
    case.loss(m, "a").backward()
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        if k in frozen:
            assert p.grad is None, k
    assert_bitwise(_grads(m), {k: v for k, v in full.items() if k not in frozen}, f"frozen subset ({rule})")


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_c7_backward_with_stale_packs_raises(case):
    m = case.build()
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    case.loss(m, "a").backward()
    loss_a = case.loss(m, "a")
    opt.step()  # in place: bumps every parameter's version counter
    loss_b = case.loss(m, "b")  # repacks the updated weights
    err, ops = launches(loss_a.backward)
    assert isinstance(err, RuntimeError), repr(err)
    assert "later forward" in str(err) and "repacked" in str(err), str(err)
    assert ops == [], ops[:3]
    opt.zero_grad(set_to_none=True)
    loss_b.backward()  # the latest forward's own backward is unaffected
    torch.cuda.synchronize()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_c7_two_forwards_then_two_backwards_without_update(case):
    ga, gb = fresh(case, "a"), fresh(case, "b")
    m = case.build()
    loss_a, loss_b = case.loss(m, "a"), case.loss(m, "b")
    loss_a.backward()
    got_a = _grads(m)
    m.zero_grad(set_to_none=True)
    loss_b.backward()
    torch.cuda.synchronize()
    assert_bitwise(got_a, ga, "backward A after forward B")
    assert_bitwise(_grads(m), gb, "backward B")


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_c8_second_backward_raises(case):
    m = case.build()
    loss = case.loss(m, "a")
    loss.backward(retain_graph=True)
    err, ops = launches(loss.backward)
    assert isinstance(err, RuntimeError), repr(err)
    assert "tape is freed after the first backward" in str(err), str(err)
    assert ops == [], ops[:3]
    torch.cuda.synchronize()
    assert_bitwise(_grads(m), fresh(case, "a"), ".grad after the refused second backward")


def _first_activation(tape_ctx):
    """The staged input of the network, saved for its backward (UNet: tape entry 0; DiT: the forward's state)."""
    if "tape" in tape_ctx:
        return tape_ctx["tape"][0][1]["xin"]
    return tape_ctx["st"]["xin"]


@pytest.mark.parametrize("name", ["cond_staged", "dit"])
def test_c9_staged_backward_releases_the_tape(name):
    case = AC.BY_NAME[name]
    m = case.build()
    m.sdmi_staged_backward = True
    loss = case.loss(m, "a")
    run = m._sdmi.last_run
    act, pred = _first_activation(run.ctx), run.shape[3]
    assert isinstance(act, torch.Tensor) and isinstance(pred, torch.Tensor)
    refs = [weakref.ref(act), weakref.ref(pred)]
    del act, pred
    loss.backward()
    torch.cuda.synchronize()
    del loss
    gc.collect()
    assert run is m._sdmi.last_run and run.handed >= 1
    assert run.ctx is None and run.shape is None and run.gviews is None and run.gen is None
    assert [r() is None for r in refs] == [True, True], "a saved activation / the prediction outlived the backward"
    assert_bitwise(_grads(m), fresh(case, "a"), "staged backward")


# ---- LPIPS: gradients go to the images --------------------------------------------------------------------------------
def _lpips():
    from models.lpips import LPIPS
    from tests import lpips_ref as R
    m = LPIPS()
    m.load_state_dict(R.seeded_state())
    ref = R.reference(2, 32, 32)
    return m.cuda(), ref["out"].cuda(), ref["im"].cuda(), ref["im"].flip(0).contiguous().cuda()


def test_lpips_image_gradients_add_up():
    m, out, im_a, im_b = _lpips()
    single = []
    for w, im in ((4.0, im_a), (1.0, im_b)):
        x = out.clone().requires_grad_(True)
        (w * m(x, im).mean()).backward()
        single.append(x.grad.clone())
    want = single[0] + single[1]
    x = out.clone().requires_grad_(True)  # C1: one graph
    (4.0 * m(x, im_a).mean() + m(x, im_b).mean()).backward()
    y = out.clone().requires_grad_(True)  # C3: two backwards
    (4.0 * m(y, im_a).mean()).backward()
    m(y, im_b).mean().backward()
    torch.cuda.synchronize()
    assert torch.equal(x.grad, want) and torch.equal(y.grad, want)


def test_lpips_second_backward_raises():
    m, out, im_a, _ = _lpips()
    x = out.clone().requires_grad_(True)
    loss = m(x, im_a).mean()
    loss.backward(retain_graph=True)
    g = x.grad.clone()
    err, ops = launches(loss.backward)
    assert isinstance(err, RuntimeError) and "tape is freed after the first backward" in str(err), repr(err)
    assert ops == [] and torch.equal(x.grad, g)
