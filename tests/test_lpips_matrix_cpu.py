"""CPU checks of tests/lpips_matrix.py: the rows against the restated host rules, the coverage table, the exact family's
margins, the index models and float64 references against torch, the measured constants K_RN, K_D and K_G, that every
perturbed reference leaves its statement, and the -1 returns of the eight entry points (host pointers: nothing is
launched)."""
import collections
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lpips_matrix as M

opt = M.opt
DIST_SHAPES = sorted({r.dims for r in M.rows_of(M.DFWD)})


def test_bindings_have_the_documented_arity():
    assert M.ARITY == {"sdmi_lpips_prep": 12, "sdmi_lpips_image_grad": 11, "sdmi_maxpool2_fwd": 7, "sdmi_maxpool2_bwd": 8,
                       "sdmi_lpips_dist_fwd": 11, "sdmi_lpips_dist_bwd": 15, "sdmi_lpips_mean": 5, "sdmi_lpips_dist_workspace": 3}


def test_rows_follow_the_restated_rules():
    for r in M.ROWS:
        assert list(r.launches) == M.expected_launches(r.entry, r.dims), M.row_id(r)
    ids = [M.row_id(r) for r in M.ROWS]
    assert len(set(ids)) == len(ids)


def test_the_restated_rules_at_known_points():
    assert [M.ppb(C) for C in (64, 128, 256, 512)] == [256, 128, 64, 32]
    assert [M.ppw(C) for C in (64, 128, 256, 512)] == [8, 4, 2, 1]
    assert M.grid_for(0) == 1 and M.grid_for(256) == 1 and M.grid_for(257) == 2
    assert M.grid_for(65536 * 256) == 65536 and M.grid_for(65536 * 256 + 1) == 65536
    assert M.work_of(M.PREP, (3, 33, 40)) == 7920 and M.work_of(M.IGRAD, (3, 33, 40)) == 3960
    assert M.work_of(M.POOLF, (2, 5, 7, 128)) == 2 * 2 * 3 * 16 and M.work_of(M.POOLB, (2, 5, 7, 128)) == 2 * 3 * 4 * 16
    assert M.workspace(1, 1, 64) == 4 and M.workspace(3, 257, 64) == 24 and M.workspace(2, 16385, 64) == 520
    assert M.workspace(2, 2049, 512) == 520 and M.blocks(101, 512) == 4
    assert M.expected_launches(M.DFWD, (3, 773, 64)) == [("lpips_dist_fwd_kernel", 12), ("lpips_dist_sum_kernel", 3)]
    assert M.expected_launches(M.DBWD, (3, 197, 256)) == [("lpips_dist_bwd_kernel", 12)]
    # the element-wise grid cap is out of reach at test size: no row claims it
    for r in M.rows_of(M.PREP, M.IGRAD, M.POOLF, M.POOLB):
        assert M.work_of(r.entry, r.dims) < M.GRID_CAP * M.NT and r.launches[0][1] < M.GRID_CAP


# ----------------------------------------------------------------------------------------------------------------
# coverage: every named need has a row, and every row is the only cover of some named need
# ----------------------------------------------------------------------------------------------------------------
def _needs():
    need = []
    add = lambda what, pred: need.append((what, pred))  # noqa: E731
    for C in M.TAP_CHANNELS:
        pw, pb = M.ppw(C), M.ppb(C)
        for entry in (M.DFWD, M.DBWD):
            for full in (0, 1):
                for B in (1, 3):
                    for what, P in (("one pixel", 1), ("a wave and a pixel", pw + 1), ("a ragged workgroup", pb - 1),
                                    ("one workgroup", pb), ("a workgroup and a pixel", pb + 1), ("several, ragged", 3 * pb + 5)):
                        add(f"{entry} C {C} {what} B {B} full {full}",
                            lambda r, e=entry, d=(B, P, C), f=full: r.entry == e and r.dims == d and opt(r, "full") == f)
                add(f"{entry} C {C} 65 partials full {full}",
                    lambda r, e=entry, C=C, f=full: r.entry == e and r.dims == (2, 64 * M.ppb(C) + 1, C) and opt(r, "full") == f)
    for entry in (M.POOLF, M.POOLB):
        add(f"{entry} one window, one group", lambda r, e=entry: r.entry == e and r.dims == (1, 2, 2, 8))
        add(f"{entry} odd H and W, one group", lambda r, e=entry: r.entry == e and r.dims == (1, 3, 3, 8))
        add(f"{entry} H = 2, odd W", lambda r, e=entry: r.entry == e and r.dims[1] == 2 and r.dims[2] % 2)
        add(f"{entry} W = 2, odd H", lambda r, e=entry: r.entry == e and r.dims[2] == 2 and r.dims[1] % 2 and r.dims[1] > 3)
        add(f"{entry} odd H and W, N > 1", lambda r, e=entry: r.entry == e and r.dims[1] % 2 and r.dims[2] % 2 and r.dims[0] > 1)
        add(f"{entry} even sides, two workgroups, C 64", lambda r, e=entry: r.entry == e and r.dims[3] == 64 and r.launches[0][1] == 2)
        add(f"{entry} C = 512", lambda r, e=entry: r.entry == e and r.dims[3] == 512)
    for dims in ((1, 1, 1), (2, 5, 7), (1, 16, 16), (3, 33, 40)):
        for a in (0, 1):
            for b in (0, 1):
                for n in (0, 1):
                    add(f"prep {dims} layouts {a}{b} normalize {n}",
                        lambda r, o=dict(nhwc0=a, nhwc1=b, normalize=n), d=dims: r.entry == M.PREP and r.dims == d and dict(r.opt) == o)
        for m in M.MODES:
            add(f"image_grad {dims} {m}", lambda r, d=dims, m=m: r.entry == M.IGRAD and r.dims == d and opt(r, "mode") == m)
    for B in (1, 3, 65):
        add(f"mean B {B}", lambda r, B=B: r.entry == M.MEAN and r.dims == (B,))
    return need


def _missing(rows, needs):
    return [what for what, pred in needs if not any(pred(r) for r in rows)]


def test_coverage():
    assert _missing(M.ROWS, _needs()) == []
    assert any(M.blocks(r.dims[1], r.dims[2]) > 64 for r in M.rows_of(M.DFWD))      # the sum kernel's second trip


def test_no_row_can_be_removed():
    needs = _needs()
    covers = collections.Counter()
    for what, pred in needs:
        hit = [r for r in M.ROWS if pred(r)]
        if len(hit) == 1:
            covers[M.row_id(hit[0])] += 1
    for r in M.ROWS:
        assert covers[M.row_id(r)], f"ROWS without {M.row_id(r)} passes every coverage check"


# ----------------------------------------------------------------------------------------------------------------
# the exact family
# ----------------------------------------------------------------------------------------------------------------
def test_exact_family_is_exact():
    seen = collections.Counter()
    for B, P, C in DIST_SHAPES:
        c = M.dist_case("exact", B, P, C)
        f = c["f"]
        tag = (B, P, C)
        assert M.bf16(f).equal(f) and M.bf16(c["addend"]).equal(c["addend"])
        n = (f != 0).sum(-1)
        assert set(n.unique().tolist()) <= {0, 1, 4, 16, 64}
        assert bool(((f == 0) | (f == f.max(-1, keepdim=True).values)).all())
        rn = M.rn_reference(c)
        assert bool((torch.log2(rn[n > 0]) == torch.log2(rn[n > 0]).round()).all()), tag     # powers of two
        assert bool((rn[n == 0] == 1e12).all())                     # (float64: the kernel's is fl32(1e12), RN_ZERO)
        d, Mx = M.pixel_terms(c)
        part = M.block_sums(d, C)
        unit = 2.0 ** -8                                            # w in quarters, (u0 - u1)^2 in 64ths
        assert bool((d / unit == (d / unit).round()).all()), tag
        assert float(d.sum(-1).max()) / unit < 2.0 ** 24 and float(M.block_sums(Mx, C).max()) / unit < 2.0 ** 24, tag
        rn32, part32 = M.emulate_forward(c)
        live = n > 0
        assert torch.equal(rn32.double()[live], rn[live]) and bool((rn32[~live] == M.RN_ZERO).all()), tag
        assert torch.equal(part32.double(), part), tag
        for full in (1, 0):
            val = M.val_from_partials(part32, P, c["prev"] if full else None).double()
            want = part.sum(-1) / P + (c["prev"] if full else 0)
            if P & (P - 1) == 0:
                assert torch.equal(val, want), tag
            else:
                assert not full or bool((c["prev"] == 0).all())
                assert torch.equal(val, (part.sum(-1).float() * M.inv_p32(P)).double()), tag
            for side in (0, 1):
                ref, T = M.dy_reference(c, side, full)
                if full or P & (P - 1) == 0:
                    assert M.is_f32(ref), (tag, full, side)         # the sum with addend is an fp32 value: one bf16 rounding
                    x, _ = M.dy_reference(c, side, full, drop_addend=True)
                    assert M.is_f32(x), (tag, full, side)
                # (a bare row off a power of two has coef = fl(1 / P): its one inexact product is rounded to fp32 once)
                assert torch.equal(M.emulate_dy(c, side, full).double(), ref.float().double()), (tag, full, side)
                if full:        # coef = 2 g exactly off a power of two, 2 g / P on one
                    assert bool((M.coef64(c, full)[:, 0] * (P if P & (P - 1) == 0 else 1) == 2.0 * c["g"].repeat_interleave(P)).all())
        same = (f[0] == f[1]).all(-1)
        z0, z1 = (f[0] == 0).all(-1), (f[1] == 0).all(-1)
        share = ((f[0] != 0) & (f[1] != 0)).any(-1)
        seen.update(identical=int((same & ~z0).sum()), zero0=int((z0 & ~z1).sum()), zero1=int((z1 & ~z0).sum()), both=int((z0 & z1).sum()),
                    share=int((share & ~same).sum()), disjoint=int((~share & ~z0 & ~z1).sum()))
        if B * P >= 6:
            assert bool((z0 & ~z1).any()) and bool((z1 & ~z0).any()) and bool((z0 & z1).any()), tag
        # identical pairs: val == +0 and dy == addend bits where a > 0
        ident = same & ~z0
        if bool(ident.any()):
            assert bool((d.reshape(-1)[ident] == 0).all())
            ref, _ = M.dy_reference(c, 0, 1)
            a = f[0][ident]
            assert torch.equal(ref[ident][a > 0], c["addend"][ident][a > 0])
    assert all(seen[k] > 50 for k in ("identical", "zero0", "zero1", "both", "share", "disjoint")), seen


def test_soft_family_domain():
    for B, P, C in DIST_SHAPES:
        c = M.dist_case("soft", B, P, C)
        f = c["f"]
        norm = f.pow(2).sum(-1).sqrt()
        assert bool(((norm == 0) | (norm >= 2.0 ** -28)).all())
        assert M.bf16(f).equal(f) and bool((f >= 0).all())
        if B * P > 4:
            assert bool((norm == 0).any()) and bool(((f[1, 0] > 0) & (f[1, 0] < 2.0 ** -28)).all())
        for r, sides in c["spots"]:
            for s in sides:
                assert bool((f[s, r] == 0).all())
        assert abs(float((f == 0).double().mean()) - 0.5) < 0.1 or B * P < 100


# ----------------------------------------------------------------------------------------------------------------
# models and references against torch
# ----------------------------------------------------------------------------------------------------------------
def _eq_nan(a, b):
    n = torch.isnan(b)
    return bool(torch.equal(torch.isnan(a), n)) and bool(torch.equal(a[~n], b[~n]))


@pytest.mark.parametrize("kind", ["ties", "special"])
def test_pool_models_against_torch(kind):
    for r in M.rows_of(M.POOLF):
        c = M.pool_case(kind, *r.dims)
        x, dy = c["x"], c["dy"]
        xt = x.permute(0, 3, 1, 2).detach().clone().requires_grad_(True)
        yt = F.max_pool2d(xt, 2, 2)
        yt.backward(dy.permute(0, 3, 1, 2))
        y, _ = M.pool_model(x)
        dx = M.pool_bwd_model(x, dy)
        assert M.same_bits(y, yt.detach().permute(0, 2, 3, 1)), (kind, r.dims)
        assert _eq_nan(dx.float(), xt.grad.permute(0, 2, 3, 1).float()), (kind, r.dims)
        H, W = r.dims[1:3]
        assert bool((M.bits(dx[:, 2 * (H // 2):].contiguous()) == 0).all()) and bool((M.bits(dx[:, :, 2 * (W // 2):].contiguous()) == 0).all())


def test_pool_special_family_holds_the_planted_windows():
    x = M.pool_case("special", 1, 2, 9, 16)["x"]
    y, arg = M.pool_model(x)
    w0 = x[0, :2, :2].reshape(4, 16).float()
    nan = torch.isnan(w0)
    for k in range(4):
        assert bool((nan[k] & (nan.sum(0) == 1)).any())              # a single NaN at each position
    assert bool((nan.sum(0) == 2).any()) and bool(torch.isnan(y[0, 0, 0].float())[nan.any(0)].all())
    assert arg[0, 0, 0, 4] == 2 and arg[0, 0, 0, 8] == 3 and arg[0, 0, 0, 0] == 0       # the last NaN
    assert M.bits(y[0, 0, 0, 5:6]) == M.bits(torch.tensor([-0.0]).bfloat16()) and M.bits(y[0, 0, 0, 6:7]) == 0   # the first zero
    assert arg[0, 0, 0, 5] == 0 and arg[0, 0, 0, 6] == 0 and arg[0, 0, 0, 7] == 0 and arg[0, 0, 0, 12] == 0
    # the perturbed models leave the statements
    for kw in (dict(last_max=True), dict(nan_rule=False)):
        _, argp = M.pool_model(x, **kw)
        assert not torch.equal(argp, arg)
    assert not M.same_bits(M.pool_model(x, nan_rule=False)[0], y)
    c = M.pool_case("ties", 3, 6, 10, 64)
    assert not M.same_bits(M.pool_bwd_model(c["x"], c["dy"], last_max=True), M.pool_bwd_model(c["x"], c["dy"]))


def test_distance_references_against_autograd():
    for B, P, C in ((3, 9, 64), (1, 129, 128), (3, 3, 256), (1, 33, 512)):
        c = M.dist_case("soft", B, P, C)
        fl = c["f"].clone().requires_grad_(True)
        u = F.normalize(fl.view(2, B, P, C), dim=-1, eps=1e-12)
        val = (((u[0] - u[1]) ** 2) * c["w"]).sum(-1).mean(-1)
        (val * c["g"] * c["gscale"]).sum().backward()
        d, _ = M.pixel_terms(c)
        assert torch.allclose(d.mean(-1), val.detach(), rtol=1e-12, atol=0)
        for side in (0, 1):
            ref, T = M.dy_reference(c, side, 1, drop_addend=True)
            # coef is the kernel's fp32 value: a relative 2^-22 away from the float64 product at most
            want = torch.where(c["f"][side] > 0, fl.grad[side], torch.zeros_like(ref))
            assert bool(((ref - want).abs() <= 2.0 ** -22 * T + 1e-300).all()), (B, P, C, side)
            assert bool((ref[(c["f"][side] == 0)] == 0).all())
        live = c["f"].pow(2).sum(-1) > 0
        assert torch.allclose(M.rn_reference(c)[live], 1 / c["f"].norm(dim=-1)[live], rtol=1e-15)


def test_elementwise_references_against_torch():
    for kind in ("soft", "special"):
        c = M.image_case(kind, 2, 5, 7)
        shift, scale = torch.tensor(M.SHIFT), torch.tensor(M.SCALE)
        for normalize in (0, 1):
            ref = M.prep_reference(c["ims"], normalize)
            assert ref.shape == (140, 8) and bool((M.bits(ref[:, 3:].contiguous()) == 0).all())
            x = c["ims"][1][1, 2, 3, 4]
            v = (np.float32(2) * x.numpy() - np.float32(1)) if normalize else x.numpy()
            want = torch.tensor((v - shift[2].numpy()) / scale[2].numpy()).bfloat16()
            assert M.same_bits(ref[70 + 35 + 3 * 7 + 4, 2].reshape(1), want.reshape(1))
            g = c["d"][:, :3].float() / scale * (2.0 if normalize else 1.0)
            out = M.image_grad_reference(c, 2, 5, 7, normalize, "nchw_acc")
            assert M.same_bits(out["nchw"][1, 2].reshape(-1), g[35:, 2].contiguous())
            assert M.same_bits(out["acc"][:, 3:], c["acc"][:, 3:]) and M.same_bits(out["acc"][:, :3], (c["acc"][:, :3].float() + g).bfloat16())
            whole = M.image_grad_reference(c, 2, 5, 7, normalize, "mse")["acc"]
            t = c["target"].permute(0, 2, 3, 1).reshape(-1, 3)
            p = c["pred"].permute(0, 2, 3, 1).reshape(-1, 3)
            assert M.same_bits(whole[:, :3], (2 * (p - t) / 210.0 + g).bfloat16()) and bool((M.bits(whole[:, 3:].contiguous()) == 0).all())
    sp = M.image_case("special", 3, 33, 40)
    for t in (sp["ims"][0], sp["d"].float(), sp["target"]):
        assert bool(torch.isnan(t).any()) and bool(torch.isinf(t).any()) and bool(((t != 0) & (t.abs() < 2.0 ** -126)).any())
        assert bool((M.bits(t.contiguous()) == -2 ** 31).any() or (M.bits(t.bfloat16().contiguous()) == -2 ** 15).any())   # -0
    c = M.mean_case("soft", 65)
    assert abs(float(M.mean_reference(c)) - float(c["val"].double().sum() * c["scale"])) < 1e-5


# ----------------------------------------------------------------------------------------------------------------
# the constants are measured
# ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ratios():
    worst = dict(rn=(0.0, None), partial=(0.0, None), dy=(0.0, None))

    def note(key, ratio, where):
        if ratio > worst[key][0]:
            worst[key] = (ratio, where)

    for B, P, C in DIST_SHAPES:
        c = M.dist_case("soft", B, P, C)
        rn32, part32 = M.emulate_forward(c)
        rn64 = M.rn_reference(c)
        live = c["f"].pow(2).sum(-1) > 0
        assert bool((rn32[~live] == M.RN_ZERO).all())
        note("rn", float(((rn32.double() - rn64).abs()[live] / (M.U24 * rn64[live])).max()), (B, P, C))
        d, Mx = M.pixel_terms(c)
        S64, Mb = M.block_sums(d, C), M.block_sums(Mx, C)
        assert bool((part32[Mb == 0] == 0).all())
        if bool((Mb > 0).any()):
            note("partial", float(((part32.double() - S64).abs()[Mb > 0] / (M.U24 * Mb[Mb > 0])).max()), (B, P, C))
        for full in (1, 0):
            for side in (0, 1):
                ref, T = M.dy_reference(c, side, full)
                x = M.emulate_dy(c, side, full).double()
                assert bool((x[T == 0] == ref[T == 0]).all())
                note("dy", float(((x - ref).abs()[T > 0] / (M.U24 * T[T > 0])).max()), (B, P, C, full, side))
    return worst


def test_constants_are_measured(ratios):
    print({k: (round(v[0], 3), v[1]) for k, v in ratios.items()})
    for key, K in (("rn", M.K_RN), ("partial", M.K_D), ("dy", M.K_G)):
        r = ratios[key][0]
        assert abs(r - M.MEASURED[key]) <= 5e-3, (key, ratios[key])
        assert 2 * r <= K <= 3 * r, (key, r, K)


# ----------------------------------------------------------------------------------------------------------------
# every perturbed reference leaves its statement
# ----------------------------------------------------------------------------------------------------------------
_PERT = [(B, P, C) for B, P, C in DIST_SHAPES if B == 3 and P == M.ppb(C) + 1]


@pytest.mark.parametrize("dims", _PERT, ids=str)
def test_perturbed_distance_references_leave_their_statements(dims):
    B, P, C = dims
    for kind in M.KINDS:
        c = M.dist_case(kind, B, P, C)
        live = c["f"].pow(2).sum(-1) > 0
        rn64, (d, Mx) = M.rn_reference(c), M.pixel_terms(c)
        S64, Mb = M.block_sums(d, C), M.block_sums(Mx, C)
        # the pair's shuffle width halved: rn and the partials leave
        rn_h, part_h = M.emulate_forward(c, half=True)
        if kind == "exact":
            assert not torch.equal(rn_h.double()[live], rn64[live]) and not torch.equal(part_h.double(), S64)
        else:
            assert float(((rn_h.double() - rn64).abs()[live] / (M.K_RN * M.U24 * rn64[live])).max()) > 1e3
            assert float(((part_h.double() - S64).abs()[Mb > 0] / (M.K_D * M.U24 * Mb[Mb > 0])).max()) > 1e3
        # 1 / P dropped in val
        part = S64.float()
        assert not torch.equal(M.val_from_partials(part, P, c["prev"], drop_inv_p=True), M.val_from_partials(part, P, c["prev"]))
        for side in (0, 1):
            ref, T = M.dy_reference(c, side, 1)
            good = M.bf16(ref)
            assert M.dy_within(good, ref, T) <= 1.0
            for name in ("other_rn", "drop_inv_p", "drop_relu", "drop_addend", "drop_proj", "swap", "half"):
                bad = M.bf16(M.dy_reference(c, side, 1, **{name: True})[0])
                if kind == "exact":
                    assert not torch.equal(bad, good), (kind, side, name)
                else:
                    assert M.dy_within(bad, ref, T) > 10.0, (kind, side, name, M.dy_within(bad, ref, T))
        # one bf16 ulp off in one element leaves the dy statement; so does a lost planted zero
        ref, T = M.dy_reference(c, 0, 1)
        off = M.bf16(ref).clone()
        i = int(ref.abs().reshape(-1).argmax())
        off.view(-1)[i] += 2 * M.ulp_bf16(ref.reshape(-1)[i:i + 1])[0]
        assert M.dy_within(off, ref, T) > 1.0


# ----------------------------------------------------------------------------------------------------------------
# error returns
# ----------------------------------------------------------------------------------------------------------------
def _cases(base, pointers):
    """Every pointer nulled in turn, every size set to 0 and to -1."""
    out = [dict(base)]
    for k, v in base.items():
        if k in pointers:
            out.append(dict(base, **{k: 0}))
        elif k not in ("side", "nhwc0", "nhwc1", "normalize", "accumulate", "ld", "ld_dy", "ld_add"):
            out += [dict(base, **{k: 0}), dict(base, **{k: -1})]
    return out


def test_entry_points_refuse_bad_arguments_before_a_launch():
    L = M._lib.lib()
    host = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(host) + 15) // 16 * 16
    Pt = lambda on: p if on else None  # noqa: E731
    refused, accepted = collections.Counter(), collections.Counter()

    def check(entry, fn, a):
        want = M.status(entry, a)
        if want == 0:
            accepted[entry] += 1                # a valid call would launch: not made here, but counted below
            return
        refused[entry] += 1
        assert fn(a) == want == -1, (entry, a)

    ptrs = lambda *ks: {k: 1 for k in ks}  # noqa: E731
    for a in _cases(dict(ptrs("in0", "in1", "shift", "scale", "out"), B=2, H=5, W=7), ("in0", "in1", "shift", "scale", "out")):
        check(M.PREP, lambda a: L.sdmi_lpips_prep(Pt(a["in0"]), 0, Pt(a["in1"]), 1, a["B"], a["H"], a["W"], Pt(a["shift"]),
                                                  Pt(a["scale"]), 1, Pt(a["out"]), None), a)
    base = dict(ptrs("d", "scale", "nchw", "acc", "pred", "target"), B=2, H=5, W=7)
    extra = [dict(base, nchw=0, acc=0), dict(base, nchw=0, acc=0, pred=0, target=0), dict(base, acc=0, pred=0, target=0),
             dict(base, nchw=0, pred=0, target=0), dict(base, pred=0, target=0)]
    for a in _cases(base, ("d", "scale", "nchw", "acc", "pred", "target")) + extra:
        check(M.IGRAD, lambda a: L.sdmi_lpips_image_grad(Pt(a["d"]), a["B"], a["H"], a["W"], Pt(a["scale"]), 0, Pt(a["nchw"]),
                                                         Pt(a["acc"]), Pt(a["pred"]), Pt(a["target"]), None), a)
    base = dict(ptrs("x", "y"), N=2, H=4, W=6, C=16)
    extra = [dict(base, H=1), dict(base, W=1), dict(base, C=4), dict(base, C=12), dict(base, C=20)]
    for a in _cases(base, ("x", "y")) + extra:
        check(M.POOLF, lambda a: L.sdmi_maxpool2_fwd(Pt(a["x"]), a["N"], a["H"], a["W"], a["C"], Pt(a["y"]), None), a)
    for a in _cases(dict(base, dy=1), ("x", "dy", "y")) + [dict(e, dy=1) for e in extra]:
        check(M.POOLB, lambda a: L.sdmi_maxpool2_bwd(Pt(a["x"]), Pt(a["dy"]), a["N"], a["H"], a["W"], a["C"], Pt(a["y"]), None), a)
    base = dict(ptrs("f", "w", "rn", "ws", "val"), ld=64, B=2, P=5, C=64)
    extra = [dict(base, C=c, ld=512) for c in (8, 32, 96, 192, 1024)] + [dict(base, ld=56), dict(base, ld=68), dict(base, ld=63),
                                                                         dict(base, B=65536), dict(base, B=65535)]
    for a in _cases(base, ("f", "w", "rn", "ws", "val")) + extra:
        check(M.DFWD, lambda a: L.sdmi_lpips_dist_fwd(Pt(a["f"]), a["ld"], Pt(a["w"]), a["B"], a["P"], a["C"], Pt(a["rn"]), Pt(a["ws"]),
                                                      0, Pt(a["val"]), None), a)
    base = dict(ptrs("f", "w", "rn", "g", "addend", "dy"), ld=72, ld_add=80, ld_dy=88, B=2, P=5, C=64, side=1)
    extra = [dict(base, C=c, ld=512, ld_add=512, ld_dy=512) for c in (8, 32, 96, 192, 1024)]
    extra += [dict(base, **{k: v}) for k in ("ld", "ld_add", "ld_dy") for v in (56, 68, 0)]
    extra += [dict(base, side=2), dict(base, side=-1), dict(base, B=65536), dict(base, addend=0, ld_add=0),
              dict(base, addend=0, ld_add=4), dict(base, side=0)]
    for a in _cases(base, ("f", "w", "rn", "g", "addend", "dy")) + extra:
        check(M.DBWD, lambda a: L.sdmi_lpips_dist_bwd(Pt(a["f"]), a["ld"], Pt(a["w"]), Pt(a["rn"]), Pt(a["g"]), 1.0, a["B"], a["P"],
                                                      a["C"], a["side"], Pt(a["addend"]), a["ld_add"], Pt(a["dy"]), a["ld_dy"], None), a)
    for a in _cases(dict(ptrs("val", "out"), B=3), ("val", "out")):
        check(M.MEAN, lambda a: L.sdmi_lpips_mean(Pt(a["val"]), a["B"], 1.0, Pt(a["out"]), None), a)
    # how many cases each entry point must refuse, and how many status() may accept (valid calls: not made here)
    assert dict(refused) == {M.PREP: 11, M.IGRAD: 13, M.POOLF: 15, M.POOLB: 16, M.DFWD: 19, M.DBWD: 27, M.MEAN: 4}, dict(refused)
    assert dict(accepted) == {M.PREP: 1, M.IGRAD: 5, M.POOLF: 1, M.POOLB: 1, M.DFWD: 3, M.DBWD: 6, M.MEAN: 1}, dict(accepted)
    # the workspace rule, and 0 for bad arguments
    for B, P, C in DIST_SHAPES:
        assert L.sdmi_lpips_dist_workspace(B, P, C) == M.workspace(B, P, C)
    for bad in ((0, 5, 64), (-1, 5, 64), (2, 0, 64), (2, -1, 64), (2, 5, 0), (2, 5, 8), (2, 5, 96), (2, 5, 1024)):
        assert L.sdmi_lpips_dist_workspace(*bad) == 0, bad
