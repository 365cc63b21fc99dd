"""CPU checks of the ADC/DAC-aware CIM layers: the fixture (the reference's own layers, tests/golden/make_golden_adda.py)
against the restatement tests/adda_ref.py, the module surface, map_weight, and the slice identities."""
import pytest
import torch

from tests import adda_ref as A

FX, META = A.load_fixture()


def _fed_by_near_tie(r, c, f):
    near = A.near_tie(r["keep"], c["cfg"], f["map"])
    fed = torch.zeros_like(r["pre"], dtype=torch.bool)
    for (key, i), v in near.items():
        mp = f["map"][key]
        fed[..., mp["start_col"]:mp["start_col"] + mp["col_num"]] |= v
    return fed


@pytest.mark.parametrize("name", list(A.CASES))
def test_fixture_forward_is_the_restatement(name):
    """Bitwise where the weight noise is 0. With weight noise the fp32 partial sums depend on the BLAS's order of
    additions: y may differ from the float64 restatement only in elements fed by an ADC input within tau of a tie."""
    c, f = A.CASES[name], FX[name]
    assert tuple(f["map"].items()) == tuple(A.split_dict(c["geo"][0], c["geo"][1], c["blocks"]).items())
    if c["cfg"]["noise_scale"] == 0:
        assert torch.equal(A.layer_grads(c, f, torch.float32)["y"], f["y"]), name
        return
    r = A.layer_grads(c, f, torch.float64)
    bad = (f["y"].double() != r["y"].float().double()) & ~_fed_by_near_tie(r, c, f)
    assert int(bad.sum()) == 0, int(bad.sum())


@pytest.mark.parametrize("name", list(A.CASES))
def test_fixture_gradients_within_the_summation_bounds(name):
    c, f = A.CASES[name], FX[name]
    b, _ = A.grad_bounds(c, f, *A.cpu_rels(c))
    rows = A.dw_rows(name, c["geo"][1])
    for k, got in (("dx", f["dx"]), ("db", f["db"]), ("dw", f["dw_rows"])):
        ref, bd = b[k]
        ref, bd = (ref[rows], bd[rows]) if k == "dw" else (ref, bd)
        worst = float(((got.double() - ref).abs() / bd.clamp_min(1e-300)).max())
        print(f"{name} {k}: worst error / bound {worst:.3f}")
        assert worst <= 1.0, (name, k, worst)
    for k in ("ds_in", "ds_w", "ds_out", "dgain"):
        ref, bd = b[k]
        print(f"{name} {k}: {abs(float(f[k]) - ref) / bd:.3f} bounds")
        assert abs(float(f[k]) - ref) <= bd, (name, k, float(f[k]), ref, bd)


def test_fixture_conditions():
    sat, seven = {}, None
    for name, c in A.CASES.items():
        r = A.layer_grads(c, FX[name], torch.float32)
        sat[name] = A.saturation(r["keep"], c["cfg"])
        if name == "c4_7slices":
            seven = [float(x.abs().max()) for x in r["keep"]["X"]]
    assert sum(0.01 <= s <= 0.5 for s in sat.values()) >= 2 and any(s == 0 for s in sat.values()), sat
    assert len(seven) == 7 and all(v > 0 for v in seven), seven
    c = A.CASES["c8_wnoise"]
    r = A.layer_grads(c, FX["c8_wnoise"], torch.float64)
    near = A.near_tie(r["keep"], c["cfg"], FX["c8_wnoise"]["map"])
    frac = sum(int(v.sum()) for v in near.values()) / sum(v.numel() for v in near.values())
    assert frac < 0.02, frac


def test_slice_identities():
    for ib, db, ranges in ((8, 5, (15, 7)), (8, 4, (7, 7, 1)), (8, 2, (1,) * 7), (5, 5, (15,))):
        q = torch.arange(-(2 ** (ib - 1) - 1), 2 ** (ib - 1)).float()
        sl = A.slices32(q, ib, db)
        assert len(sl) == len(ranges)
        assert torch.equal(sum(s * 2 ** (i * (db - 1)) for i, s in enumerate(sl)), q)
        assert [float(s.abs().max()) for s in sl] == [float(r) for r in ranges]
        ref = A.split(q.clone(), ib, db - 1)
        assert all(torch.equal(a, b) for a, b in zip(sl, ref))


def test_module_surface_and_mapping():
    import sdmi.layers_qn_lsq_adda_cim as M
    c = A.CASES["c1_ref"]
    lin = M.Linear_lsq_adda_cim(1300, 96, bias=True, **c["cfg"])
    conv = M.Conv2d_lsq_adda_cim(72, 24, 1, 1, 0, 1, bias=True, **A.CASES["c3_conv"]["cfg"])
    assert list(lin.state_dict()) == META["linear.state_dict_keys"].split(",")
    assert list(conv.state_dict()) == META["conv.state_dict_keys"].split(",")
    for attr in ("adc_gain_min", "adc_gain_max", "adc_adjust_mode", "gain_noise", "offset_noise", "bit_slices",
                 "slice_bit", "use_FP", "update_para", "refresh_adc_params"):
        assert hasattr(lin, attr) and hasattr(conv, attr), attr
    assert (lin.bit_slices, lin.slice_bit) == (2, 4)
    net = torch.nn.Sequential(lin)
    got = M.map_weight(net, c["blocks"])["0"]
    assert list(got.items()) == list(FX["c1_ref"]["map"].items()) and lin.name == "0"
    with pytest.raises(NotImplementedError, match="kernel_size=3"):
        M.Conv2d_lsq_adda_cim(8, 8, 3, 1, 1, 1, bias=True, **c["cfg"])
    lin.update_para(input_bit=5, dac_bit=3)
    assert (lin.bit_slices, lin.slice_bit) == (2, 2)


PERTURBATIONS = ("clamp_R", "adc_recombined", "merged", "no_mask", "twos")
GRADS = ("dx", "dw", "ds_in", "ds_w", "dgain")
# (case, perturbation) pairs that neither y nor a gradient bound can catch. c5_gain has no saturated ADC input at all
# (the fixture's condition "at least one case has none"): a moved clamp edge or a dropped mask changes nothing there. The test asserts these stay blind, so the list cannot rot.
BLIND = {("c5_gain", "clamp_R"), ("c5_gain", "no_mask")}
_BOUNDS = {}


def _bounds(name):
    if name not in _BOUNDS:
        _BOUNDS[name] = A.grad_bounds(A.CASES[name], FX[name])[0]
    return _BOUNDS[name]


def _leaves(name, r):
    """Which of y and GRADS of a run leave the fixture (y, bitwise where there is no weight noise) or the HIP path's
    derived bounds around the float64 restatement."""
    c, f, b = A.CASES[name], FX[name], _bounds(name)
    out = []
    if c["cfg"]["noise_scale"] == 0 and not torch.equal(r["y"].float(), f["y"]):
        out.append("y")
    for k in GRADS:
        ref, bd = b[k]
        got = r[k].double()
        if bool(((got - ref).abs() > bd).any()) if torch.is_tensor(ref) else abs(float(got) - ref) > bd:
            out.append(k)
    return out


@pytest.mark.parametrize("name", list(A.CASES))
def test_perturbed_restatements_leave_the_bounds(name):
    """Every perturbed restatement must miss y or leave a derived gradient bound on every case, the BLIND pairs aside;
    the unperturbed one leaves none."""
    c, f = A.CASES[name], FX[name]
    assert _leaves(name, A.layer_grads(c, f, torch.float64)) == []
    for perturb in PERTURBATIONS:
        left = _leaves(name, A.layer_grads(c, f, torch.float64, perturb=perturb))
        print(f"{name} {perturb}: leaves {left}")
        assert bool(left) != ((name, perturb) in BLIND), (name, perturb, left)


@pytest.mark.parametrize("name", ("c1_ref", "c2_small", "c3_conv", "c4_7slices", "c6_adcnoise"))
def test_gradient_identities(name):
    """d x_q[block j] = (as / L) (dZ o M_j) @ W2[block j]^T, d W2[block j] = as sum_i 2^(i sb) X_i[block j]^T @ (dZ o
    mask_ij) and d as = sum dZ o T - (1 / as) sum d_pre o (pre - bias), against autograd of the restatement (float64)."""
    c, f = A.CASES[name], FX[name]
    cfg = c["cfg"]
    r = A.layer_grads(c, f, torch.float64)
    k = r["keep"]
    nL, sb, R = A.n_slices(cfg["input_bit"], cfg["dac_bit"]), cfg["dac_bit"] - 1, 2 ** (cfg["adc_bit"] - 1) - 1
    a_s, ws, is_ = float(k["a_s"]), 1 / float(f["s_w"]), 1 / float(f["s_in"])
    dpre = A.rows_of(c["kind"], r["d_pre"])
    dZ = dpre / a_s / is_ / ws
    W2 = k["wq"].reshape(k["wq"].shape[0], -1).t()
    dxq, dW2, T = torch.zeros_like(k["X"][0]), torch.zeros_like(W2), torch.zeros_like(dZ)
    blocks = sorted({(m["start_row"], m["row_num"]) for m in f["map"].values()})
    for r0, rn in blocks:
        M = torch.zeros_like(dZ)
        for key, m in f["map"].items():
            if m["start_row"] != r0:
                continue
            c0, cn = m["start_col"], m["col_num"]
            for i in range(nL):
                A_ = k["A"][(key, i)]
                mask = ((A_ >= -R - 1) & (A_ <= R)).double()
                M[..., c0:c0 + cn] += mask
                g = dZ[..., c0:c0 + cn] * mask
                dW2[r0:r0 + rn, c0:c0 + cn] += a_s * 2 ** (i * sb) * (k["X"][i][..., r0:r0 + rn].reshape(-1, rn).t()
                                                                      @ g.reshape(-1, cn))
                T[..., c0:c0 + cn] += 2 ** (i * sb) * mask * k["P"][(key, i)]
        dxq[..., r0:r0 + rn] = (a_s / nL) * ((dZ * M) @ W2[r0:r0 + rn].t())
    auto_x = A.rows_of(c["kind"], k["xq_t"].grad)
    assert float((dxq - auto_x).abs().max()) <= 1e-12 * float(auto_x.abs().max())
    auto_w = k["wq_t"].grad.reshape(W2.shape[1], -1).t()
    assert float((dW2 - auto_w).abs().max()) <= 1e-12 * float(auto_w.abs().max())
    bias = f["b"].double().view(1, -1, 1, 1) if c["kind"] == "conv" else f["b"].double()
    d_as = float((dZ * T).sum()) - float((r["d_pre"] * (r["pre"] - bias)).sum()) / a_s
    leaf = f["gain"].double().clone().requires_grad_(True)
    A.adc_scale_of(leaf, cfg).backward()
    assert abs(d_as * float(leaf.grad) - float(r["dgain"])) <= 1e-9 * max(abs(float(r["dgain"])), 1e-3)


@pytest.mark.parametrize("bit", (4, 8))
def test_isint_backward_is_the_plain_backward_on_the_gradient_over_the_step(bit):
    """x_q = q se / se.detach(): its gradients in x and in the step are the isint=False quantiser's on g / se."""
    from tests import lsq_ref as LR
    gen = torch.Generator().manual_seed(bit)
    x = torch.randn(300, generator=gen, dtype=torch.float64)
    g = torch.randn(300, generator=gen, dtype=torch.float64)
    step = torch.tensor(2.4 / LR.qp_of(bit), dtype=torch.float64)  # a few elements beyond +-Qp
    grads = []
    for fn, up in ((A.quant_int, g), (lambda a, b_, s: LR.quant_lsq(a, b_, s), g / LR.effective_step(step, bit, 300))):
        xr, sr = x.clone().requires_grad_(True), step.clone().requires_grad_(True)
        fn(xr, bit, sr).backward(up)
        grads.append((xr.grad, sr.grad))
    assert torch.allclose(grads[0][0], grads[1][0], rtol=1e-13, atol=0)
    assert torch.allclose(grads[0][1], grads[1][1], rtol=1e-12, atol=0)


def test_convert_and_register():
    import types
    import sdmi.layers_qn_lsq as Q
    import sdmi.layers_qn_lsq_adda_cim as M
    nn = torch.nn
    cfg = A.CASES["c1_ref"]["cfg"]
    net = nn.Sequential(nn.Conv2d(6, 8, 1, bias=False), nn.ReLU(), nn.Flatten(), nn.Linear(8, 4),
                        Q.Linear_qn_lsq(4, 4, weight_bit=4, input_bit=8, output_bit=8, noise_scale=0.0, bias=True))
    net[4].step_size_input.data = torch.tensor(0.25)
    net[4].name = "last"
    w, b = net[3].weight, net[3].bias
    assert M.convert(net, exclude=["4"], **cfg) == ["0", "3"]
    assert type(net[0]) is M.Conv2d_lsq_adda_cim and type(net[3]) is M.Linear_lsq_adda_cim and net[0].bias is None
    assert net[3].weight is w and net[3].bias is b  # the same Parameter objects
    assert M.convert(net, assign=["4"], **cfg) == ["4"]
    assert float(net[4].step_size_input) == 0.25 and net[4].name == "last"  # copy_lsq_data, copy_meta_info
    with pytest.raises(ValueError):
        M.convert(net, exclude=["0"], assign=["3"], **cfg)
    with pytest.raises(NotImplementedError, match="kernel_size"):
        M.convert(nn.Sequential(nn.Conv2d(4, 4, 3, padding=1)), **cfg)
    reg = types.SimpleNamespace(conv_layers=(Q.Conv2d_qn_lsq, nn.Conv2d), linear_layers=(Q.Linear_qn_lsq, nn.Linear),
                                adda_layers=(), cim_layers=(), custom_layers=(Q.Linear_qn_lsq,), op_layers=(nn.Linear,),
                                adda_linear_layers=(), adda_conv_layers=(), cim_linear_layers=(), cim_conv_layers=(),
                                custom_conv_layers=(), custom_linear_layers=())
    M.register(reg)
    M.register(reg)  # twice: no duplicates
    assert reg.conv_layers == (M.Conv2d_lsq_adda_cim, Q.Conv2d_qn_lsq, nn.Conv2d)
    assert reg.linear_layers[0] is M.Linear_lsq_adda_cim and reg.adda_layers == (M.Conv2d_lsq_adda_cim, M.Linear_lsq_adda_cim)
    for name in ("cim_layers", "custom_layers", "op_layers"):
        assert getattr(reg, name)[:2] == (M.Linear_lsq_adda_cim, M.Conv2d_lsq_adda_cim), name
    # the reference's convert_to_layers takes the first class whose module path holds the layer type's name
    assert "layers_qn_lsq_adda_cim" in reg.linear_layers[0].__module__.split(".")
