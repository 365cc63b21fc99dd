"""Every kernel of csrc/misc.hip (but add_noise) and csrc/leafops.hip at every row of tests/stage_matrix.py ROWS, exact,
guarded.

The recorded launch plan must name the row's kernels and grids. Every operand and output is a window of a NaN-filled
buffer; after a call nothing but the declared outputs may have changed, bit for bit. Then the statements of
tests/stage_matrix.py, no element excluded: the movers, converters, packers, ReLU, the class-map staging, the exact
families and the MSE gradient bitwise; everything else within its measured bound. A second identical call gives
identical bits. Each bounded test prints its worst error / bound."""
import ctypes

import pytest
import torch

from tests import stage_matrix as M

pytestmark = pytest.mark.gpu
ptr, opt = M.ptr, M.opt
WORST = {}


def _L():
    from sdmi import _lib
    return _lib.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(L, call, want, tag, check=True):
    if check:
        rc, ops = M.recorded(L, call)
        assert rc == 0, f"{tag}: returned {rc}"
        assert M.launches_match(ops, want), f"{tag}: launched {ops[:6]} ({len(ops)}), the matrix says {list(want)[:6]}"
    else:
        assert call() == 0, tag
    torch.cuda.synchronize()


def _unchanged(g, tag):
    bad = g.changed()
    assert bad is None, f"{tag}: changed outside the outputs: {bad}"


def _same(got, ref, what, tag):
    assert got.shape == ref.shape and M.eq_bits(got, ref), f"{tag}: {what} differs from its bitwise value in " \
        f"{M.n_diff(got, ref) if got.shape == ref.shape else 'shape'} elements"


def _within(got, ref, lim, what, tag, fine=None):
    """fine (bf16 outputs): the fp32 part K u T of the bound; the share of it in use beyond the half ulp is printed."""
    w = M.worst(got, ref, lim)
    WORST[what] = max(WORST.get(what, 0.0), w)
    more = "" if fine is None else f", (err - ulp_bf16 / 2) / (K u T) at most {M.excess(got, ref, lim.double() - fine, fine):.3f}"
    print(f"{tag}: {what} worst err / bound {w:.3f} (so far {WORST[what]:.3f}){more}")
    assert w <= 1.0, f"{tag}: {what} leaves its bound: worst err / bound {w}"


def _whole(w):
    return [(0, w.n)]


def _guard(inputs, outputs):
    g = M.Guard()
    for name, w in inputs.items():
        if w is not None:
            g.add(name, w)
    for name, (w, writable) in outputs.items():
        g.add(name, w, writable)
    return g


def _twice(once, tag):
    """once(check_launches) -> dict of CPU tensors: run it twice on fresh buffers; the second call repeats every bit."""
    first = once(True)
    again = once(False)
    for k, v in first.items():
        assert M.eq_bits(again[k], v), f"{tag}: a second identical call gives other {k}"
    return first


# ----------------------------------------------------------------------------------------------------------------
# pure data movement and conversion
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", M.rows_of(M.N2C), ids=M.row_id)
def test_nhwc_to_nchw_rows(row):
    L, tag = _L(), M.row_id(row)
    B, C, HW, ld = row.dims
    src, want = M.n2c_case(row)

    def once(check):
        S, D = M.dev(src), M.Win(B * C * HW, "cuda")
        g = _guard(dict(src=S), dict(dst=(D, _whole(D))))
        _run(L, lambda: L.sdmi_nhwc_to_nchw(ptr(S.data), opt(row, "f32"), ld, B, C, HW, ptr(D.data), _stream()),
             row.launches, tag, check)
        _unchanged(g, tag)
        return dict(dst=M.host(D, B, C, HW))

    _same(_twice(once, tag)["dst"], want, "the NCHW tensor", tag)


@pytest.mark.parametrize("row", M.rows_of(M.C2N), ids=M.row_id)
def test_nchw_to_nhwc_rows(row):
    L, tag = _L(), M.row_id(row)
    B, C, HW, ld = row.dims
    src, want = M.c2n_case(row)

    def once(check):
        S, D = M.dev(src), M.Win(B * HW * ld, "cuda", torch.bfloat16)
        g = _guard(dict(src=S), dict(dst=(D, _whole(D))))
        _run(L, lambda: L.sdmi_nchw_to_nhwc_bf16(ptr(S.data), B, C, HW, ptr(D.data), ld, _stream()), row.launches, tag, check)
        _unchanged(g, tag)
        return dict(dst=M.host(D, B * HW, ld))

    got = _twice(once, tag)["dst"]
    _same(got, want, "the NHWC tensor", tag)
    assert bool((M.bits(got[:, C:].contiguous()) == 0).all()), f"{tag}: a pad column is not +0"


@pytest.mark.parametrize("row", M.rows_of(M.SLICE), ids=M.row_id)
def test_copy_slice_rows(row):
    L, tag = _L(), M.row_id(row)
    P, C, lds, ldd = row.dims
    src, dst, want = M.slice_case(row)

    def once(check):
        S, sw = M.dev_buf(src, lds)
        D, dw = M.dev_buf(dst, ldd)
        g = _guard(dict(src=S), dict(dst=(D, [("w", 0, C)])))
        _run(L, lambda: L.sdmi_copy_slice(ptr(sw), lds, ptr(dw), ldd, P, C, opt(row, "acc"), _stream()), row.launches, tag,
             check)
        _unchanged(g, tag)
        return dict(dst=dw.cpu())

    _same(_twice(once, tag)["dst"], want, "the destination rows (columns past C included)", tag)


@pytest.mark.parametrize("row", M.rows_of(M.RELU), ids=M.row_id)
def test_relu_rows(row):
    L, tag = _L(), M.row_id(row)
    n, bwd = row.dims[0], opt(row, "bwd")
    x, dy = M.relu_case(n)
    want = M.relu_model(x, dy if bwd else None)

    def once(check):
        X, DY, Y = M.dev(x), M.dev(dy), M.Win(n, "cuda")
        g = _guard(dict(x=X, dy=DY), dict(y=(Y, _whole(Y))))
        _run(L, lambda: L.sdmi_relu(ptr(X.data), ptr(DY.data) if bwd else None, ptr(Y.data), n, _stream()), row.launches,
             tag, check)
        _unchanged(g, tag)
        return dict(y=M.host(Y))

    got = _twice(once, tag)["y"]
    _same(got, want, "the result (a NaN input gives NaN forward and passes dy backward; both zeros give +0)", tag)


@pytest.mark.parametrize("row", M.rows_of(M.RESIZE), ids=M.row_id)
def test_resize_nearest_rows(row):
    L, tag = _L(), M.row_id(row)
    BC, IH, IW, OH, OW = row.dims
    x, want = M.resize_case(row)

    def once(check):
        X, Y = M.dev(x), M.Win(BC * OH * OW, "cuda")
        g = _guard(dict(x=X), dict(y=(Y, _whole(Y))))
        _run(L, lambda: L.sdmi_resize_nearest(ptr(X.data), BC, IH, IW, ptr(Y.data), OH, OW, _stream()), row.launches, tag,
             check)
        _unchanged(g, tag)
        return dict(y=M.host(Y, BC, OH, OW))

    _same(_twice(once, tag)["y"], want, "the resized planes", tag)


@pytest.mark.parametrize("row", M.rows_of(M.CHAN), ids=M.row_id)
def test_chan_copy_rows(row):
    L, tag = _L(), M.row_id(row)
    B, C, P, sC, sc0, dC, dc0 = row.dims
    src, dst, want = M.chan_case(row)

    def once(check):
        S, D = M.dev(src), M.dev(dst)
        g = _guard(dict(src=S), dict(dst=(D, [((b * dC + dc0) * P, (b * dC + dc0 + C) * P) for b in range(B)])))
        _run(L, lambda: L.sdmi_chan_copy(ptr(S.data), sC, sc0, ptr(D.data), dC, dc0, B, C, P, _stream()), row.launches, tag,
             check)
        _unchanged(g, tag)
        return dict(dst=M.host(D, B, dC, P))

    _same(_twice(once, tag)["dst"], want, "the destination tensor", tag)


# ----------------------------------------------------------------------------------------------------------------
# weight packing
# ----------------------------------------------------------------------------------------------------------------
def _pack_once(L, row, check):
    from sdmi import _lib
    tag, descs = M.row_id(row), opt(row, "descs")
    arr = (_lib.PackDesc * len(descs))()
    srcs, dsts = [], []
    for j, d in enumerate(descs):
        dd = dict(d)
        so, si, skh, skw, kh_off, kh_mul, kw_off, kw_mul, _ = M.pack_strides(d)
        row_w = dd["KH"] * dd["KW"] * dd["Ipad"]
        S = M.dev(M.pack_source(d, j), off=dd.get("src_off", 0) // 4)
        D = M.Buf(dd["O"], dd.get("dst_ld", 0) or row_w, torch.bfloat16, "cuda")
        w = D.window(dd.get("col0", 0), row_w)
        assert w.data_ptr() % 16 == 0 and S.data.data_ptr() % 16 == dd.get("src_off", 0)
        a = arr[j]
        a.src, a.dst = S.data.data_ptr(), w.data_ptr()
        a.so, a.si, a.skh, a.skw = so, si, skh, skw
        a.O, a.I, a.Ipad, a.KH, a.KW = dd["O"], dd["I"], dd["Ipad"], dd["KH"], dd["KW"]
        a.kh_off, a.kh_mul, a.kw_off, a.kw_mul, a.dst_ld = kh_off, kh_mul, kw_off, kw_mul, dd.get("dst_ld", 0)
        srcs.append(S)
        dsts.append((D, w, dd.get("col0", 0), row_w))
    bmap = M.pack_bmap(descs)
    DS = M.Bytes(bytes(arr))
    BM = M.Bytes(torch.tensor(bmap, dtype=torch.int32).numpy().tobytes())
    g = M.Guard()
    g.add("descs", DS)
    g.add("bmap", BM)
    for j, S in enumerate(srcs):
        g.add(f"src{j}", S)
    for j, (D, w, col0, row_w) in enumerate(dsts):
        g.add(f"dst{j}", D, [("w", col0, row_w)])
    _run(L, lambda: L.sdmi_pack_weights(ptr(DS.data), ptr(BM.data), len(bmap), _stream()), row.launches, tag, check)
    _unchanged(g, tag)
    return {f"dst{j}": w.cpu() for j, (D, w, col0, row_w) in enumerate(dsts)}


@pytest.mark.parametrize("row", M.rows_of(M.PACK), ids=M.row_id)
def test_pack_weights_rows(row):
    L, tag = _L(), M.row_id(row)
    got = _twice(lambda check: _pack_once(L, row, check), tag)
    for j, d in enumerate(opt(row, "descs")):
        _same(got[f"dst{j}"], M.pack_model(d, M.pack_source(d, j)), f"descriptor {j}'s packed rows", tag)


def test_pack_misaligned_source_gives_the_bits_of_the_fast_path():
    L = _L()
    a, b = (r for r in M.rows_of(M.PACK) if len(opt(r, "descs")) == 1 and dict(opt(r, "descs")[0])["O"] == 57)
    assert M.eq_bits(_pack_once(L, a, False)["dst0"], _pack_once(L, b, False)["dst0"])


def _tpack_once(L, row, check):
    from sdmi import _lib
    tag, descs = M.row_id(row), opt(row, "descs")
    arr = (_lib.TPackDesc * len(descs))()
    srcs, dsts = [], []
    for j, d in enumerate(descs):
        dd = dict(d)
        src_ld, src_tap, dst_ld, dst_tap = M.tpack_dims(d)
        S = M.dev(M.tpack_source(d, j))
        D = M.Buf(dd["I"], dst_ld, torch.bfloat16, "cuda")
        base = D.window(0, dst_ld)
        assert base.data_ptr() % 16 == 0 and S.data.data_ptr() % 16 == 0
        a = arr[j]
        a.src, a.dst = S.data.data_ptr(), base.data_ptr()
        a.O, a.I, a.taps = dd["O"], dd["I"], len(dd["smap"])
        a.src_ld, a.src_tap, a.dst_ld, a.dst_tap = src_ld, src_tap, dst_ld, dst_tap
        for t, v in enumerate(dd["smap"]):
            a.smap[t] = v
        srcs.append(S)
        dsts.append((D, dd, dst_tap))
    tmap = M.tpack_bmap(descs)
    DS = M.Bytes(bytes(arr))
    BM = M.Bytes(torch.tensor(tmap, dtype=torch.int32).numpy().tobytes())
    g = M.Guard()
    g.add("descs", DS)
    g.add("tmap", BM)
    for j, S in enumerate(srcs):
        g.add(f"src{j}", S)
    for j, (D, dd, dst_tap) in enumerate(dsts):
        g.add(f"dst{j}", D, [("w", t * dst_tap, dd["O"]) for t in range(len(dd["smap"]))])
    _run(L, lambda: L.sdmi_pack_transpose(ptr(DS.data), ptr(BM.data), len(tmap), _stream()), row.launches, tag, check)
    _unchanged(g, tag)
    return {f"dst{j}": torch.stack([D.window(t * dst_tap, dd["O"]).cpu() for t in range(len(dd["smap"]))], 1)
            for j, (D, dd, dst_tap) in enumerate(dsts)}


@pytest.mark.parametrize("row", M.rows_of(M.TPACK), ids=M.row_id)
def test_pack_transpose_rows(row):
    L, tag = _L(), M.row_id(row)
    got = _twice(lambda check: _tpack_once(L, row, check), tag)
    for j, d in enumerate(opt(row, "descs")):
        _same(got[f"dst{j}"], M.tpack_model(d, M.tpack_source(d, j)), f"descriptor {j}'s transposed taps", tag)


def test_the_packers_launch_nothing_for_no_blocks():
    L = _L()
    for fn in (L.sdmi_pack_weights, L.sdmi_pack_transpose):
        for n in (0, -1):
            rc, ops = M.recorded(L, lambda: fn(None, None, n, _stream()))
            assert rc == 0 and ops == [], (n, rc, ops)


# ----------------------------------------------------------------------------------------------------------------
# input staging and the conditioning weight gradient
# ----------------------------------------------------------------------------------------------------------------
def _mask_operand(c, cmap):
    if c["mask"] is None:
        return None
    return M.Bytes(c["mask"].numpy().tobytes()) if cmap else M.dev(c["mask"])


@pytest.mark.parametrize("row", M.rows_of(M.PREP), ids=M.row_id)
def test_prep_input_rows(row):
    L, tag = _L(), M.row_id(row)
    B, cx, H, W, cpad = row.dims
    kind, cmi, cmo = opt(row, "mask"), opt(row, "cmi", 0), opt(row, "cmo", 0)
    _, _, _, MH, MW = M._mask_dims(row)
    c = M.prep_case(row)
    ref = M.prep_reference(row, c)

    def once(check):
        X, MK = M.dev(c["x"]), _mask_operand(c, kind == "cmap")
        Wc = M.dev(c["w"]) if c["w"] is not None else None
        KP = M.dev(c["keep"]) if c["keep"] is not None else None
        O = M.Win(B * H * W * cpad, "cuda", torch.bfloat16)
        g = _guard(dict(x=X, mask=MK, w=Wc, keep=KP), dict(out=(O, _whole(O))))
        fn = L.sdmi_prep_input_cmap if kind == "cmap" else L.sdmi_prep_input
        p = lambda w: ptr(w.data) if w is not None else None  # noqa: E731
        if kind is None:
            call = lambda: fn(p(X), B, cx, H, W, None, 0, 1, 1, None, 0, p(O), cpad, None, _stream())  # noqa: E731
        else:
            call = lambda: fn(p(X), B, cx, H, W, p(MK), cmi, MH, MW, p(Wc), cmo, p(O), cpad, p(KP), _stream())  # noqa: E731
        _run(L, call, row.launches, tag, check)
        _unchanged(g, tag)
        return dict(out=M.host(O, B * H * W, cpad))

    got = _twice(once, tag)["out"]
    if kind == "soft":
        keep = [k for k in range(cpad) if not cx <= k < cx + cmo]
        _same(got[:, keep].contiguous(), ref["exact"][:, keep].contiguous(), "x and the zero columns", tag)
        _within(got[:, cx:cx + cmo], ref["ref"], M.prep_bound(ref["ref"], ref["T"]), "prep mask columns", tag,
                M.K_PREP * M.U24 * ref["T"])
    else:
        _same(got, ref["exact"], "the staged rows", tag)


def _cw_once(L, row, c, form, check, launches=None):
    B, H, W, cmo, cmi = row.dims
    _, _, _, MH, MW = M._mask_dims(row)
    tag = f"{M.row_id(row)} {form}"
    DX = M.dev(c["dx"])
    MK = M.Bytes(c["cmap"].numpy().tobytes()) if form == "cmap" else M.dev(c["mask"])
    KP = M.dev(c["keep"]) if c["keep"] is not None else None
    DW = M.Win(cmo * cmi, "cuda")
    g = _guard(dict(dxin=DX, mask=MK, keep=KP), dict(dw=(DW, _whole(DW))))
    fn = L.sdmi_cond_wgrad_cmap if form == "cmap" else L.sdmi_cond_wgrad
    _run(L, lambda: fn(ptr(DX.data), M.CW_LD, M.CW_CX, B, H, W, ptr(MK.data), cmi, MH, MW, cmo, ptr(DW.data),
                       ptr(KP.data) if KP is not None else None, _stream()), launches, tag, check)
    _unchanged(g, tag)
    return dict(dw=M.host(DW))


@pytest.mark.parametrize("row", M.rows_of(M.CW), ids=M.row_id)
def test_cond_wgrad_rows(row):
    L, tag = _L(), M.row_id(row)
    c = M.cw_case(row)
    ref, T = M.cw_reference(row, c)
    got = _twice(lambda check: _cw_once(L, row, c, "onehot", check, row.launches[:2]), tag)["dw"]
    if opt(row, "family") == "exact":
        _same(got, ref.float(), "dw of the one-hot form (integer sums)", tag)
        cm = _twice(lambda check: _cw_once(L, row, c, "cmap", check, row.launches[2:]), tag)["dw"]
        _same(cm, ref.float(), "dw of the class-map form", tag)
        _same(cm, got, "the class-map form against the one-hot form", tag)
    else:
        _within(got, ref, M.K_CW * M.U24 * T, "cond_wgrad", tag)


def test_cond_wgrad_nine_calls_wrap_the_partial_slots():
    L = _L()
    row = next(r for r in M.rows_of(M.CW) if r.dims == (1, 3, 11, 2, 3) and opt(r, "family") == "exact")
    assert 9 > M.CW_SLOTS
    for k in range(9):
        c = M.cw_case(row, seed=k + 1)
        ref, _ = M.cw_reference(row, c)
        form = "cmap" if k % 2 else "onehot"
        got = _cw_once(L, row, c, form, True, row.launches[2:] if k % 2 else row.launches[:2])["dw"]
        _same(got, ref.float(), f"dw of call {k}", M.row_id(row))


# ----------------------------------------------------------------------------------------------------------------
# the loss
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ("exact", "soft"))
@pytest.mark.parametrize("row", M.rows_of(M.MSE), ids=M.row_id)
def test_mse_rows(row, family):
    L, tag = _L(), f"{M.row_id(row)} {family}"
    B, C, HW, ld = row.dims
    c = M.mse_case(row, family)
    ref = M.mse_reference(row, c)
    blocks = M.mse_blocks(B * HW * ld)
    assert L.sdmi_mse_workspace() == M.mse_workspace()
    with_grad, gdev = opt(row, "grad", 1), opt(row, "gdev", 0)

    def once(check):
        P, T = M.dev(c["pred"]), M.dev(c["target"])
        GS = M.dev(torch.tensor([c["gscale"]]))
        G = M.Win(B * HW * ld, "cuda", torch.bfloat16)
        WS, LS = M.Win(M.mse_workspace() // 4, "cuda"), M.Win(1, "cuda")
        g = _guard(dict(pred=P, target=T, gscale=GS),
                   dict(grad=(G, _whole(G) if with_grad else []), ws=(WS, [(0, blocks)]), loss=(LS, _whole(LS))))
        # by value the kernel must ignore nothing; from the device the value passed is a decoy
        _run(L, lambda: L.sdmi_mse(ptr(P.data), ld, ptr(T.data), B, C, HW, -7.0 if gdev else c["gscale"],
                                   ptr(GS.data) if gdev else None, ptr(G.data) if with_grad else None, ptr(WS.data),
                                   ptr(LS.data), _stream()), row.launches, tag, check)
        _unchanged(g, tag)
        return dict(grad=M.host(G, B * HW, ld), loss=M.host(LS), ws=M.host(WS)[:blocks])

    out = _twice(once, tag)
    if with_grad:
        _same(out["grad"], M.mse_grad_model(row, c), "the gradient (pad columns +0)", tag)
    loss = out["loss"].double()
    if family == "exact" and M.mse_exact(row):
        assert float(loss) == ref, f"{tag}: the loss {float(loss)} is not the exact {ref}"
    f64 = lambda v: torch.tensor([v], dtype=torch.float64)  # noqa: E731
    _within(loss, f64(ref), f64(M.K_MSE * M.U24 * ref), f"mse loss ({family})", tag)


# ----------------------------------------------------------------------------------------------------------------
# time embedding
# ----------------------------------------------------------------------------------------------------------------
def _temb_once(L, row, t, f32, check):
    B, dim, ld = row.dims
    tag = M.row_id(row)
    tstride = opt(row, "tstride", 1)
    TT = M.Bytes(t.numpy().tobytes())
    O = M.Buf(B, ld, torch.bfloat16, "cuda")
    F32 = M.Win(B * dim, "cuda")
    g = M.Guard()
    g.add("t", TT)
    g.add("out", O, [("w", 0, dim)])
    g.add("out_f32", F32, _whole(F32) if f32 else [])
    _run(L, lambda: L.sdmi_time_embedding(ptr(TT.data), tstride, B, dim, ptr(O.window(0, dim)), ld,
                                          ptr(F32.data) if f32 else None, _stream()), row.launches, tag, check)
    _unchanged(g, tag)
    return dict(out=O.window(0, dim).cpu(), f32=M.host(F32, B, dim))


@pytest.mark.parametrize("row", M.rows_of(M.TEMB), ids=M.row_id)
def test_time_embedding_rows(row):
    L, tag = _L(), M.row_id(row)
    B, dim, ld = row.dims
    ts = M.temb_t(row)
    calls = [ts] if opt(row, "tstride", 1) else [ts[i:i + 1] for i in range(len(ts))]
    for t in calls:
        assert len(t) == (B if opt(row, "tstride", 1) else 1)
        full = t if opt(row, "tstride", 1) else t.repeat(B)
        ref, a = M.temb_reference(full, dim)
        out = _twice(lambda check: _temb_once(L, row, t, True, check), tag)
        _within(out["f32"], ref, M.temb_bound(a), "time embedding fp32", tag)
        _same(out["out"], out["f32"].bfloat16(), "the bf16 output against RNE of the kernel's own fp32 output", tag)
        if not opt(row, "f32", 1):
            alone = _twice(lambda check: _temb_once(L, row, t, False, check), tag)
            _same(alone["out"], out["out"], "the bf16 output of a call without out_f32", tag)
        if opt(row, "t") == M.TGOLD:
            gold = M.golden_temb()[f"emb{dim}"].double()
            _within(gold, ref, M.temb_bound(a), "golden time embedding against float64", tag)
            print(f"{tag}: largest difference from the golden fp32 values {float((out['f32'].double() - gold).abs().max()):.3e}")


# ----------------------------------------------------------------------------------------------------------------
# SiLU on every bf16 bit pattern
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", M.rows_of(M.SILU), ids=M.row_id)
def test_silu_rows(row):
    L, tag = _L(), M.row_id(row)
    n, bwd = row.dims[0], opt(row, "bwd")
    x = M.silu_x()
    dyv = M.SILU_DY[opt(row, "dy")] if bwd else None
    dy = torch.full((n,), dyv if bwd else 0.0).bfloat16()

    def once(check):
        X, DY, Y = M.dev(x), M.dev(dy), M.Win(n, "cuda", torch.bfloat16)
        g = _guard(dict(x=X, dy=DY), dict(y=(Y, _whole(Y))))
        _run(L, lambda: L.sdmi_silu(ptr(X.data), ptr(DY.data) if bwd else None, ptr(Y.data), n, _stream()), row.launches,
             tag, check)
        _unchanged(g, tag)
        return dict(y=M.host(Y))

    got = _twice(once, tag)["y"]
    ref, T = M.silu_reference(x, dyv)
    carved = M.silu_carved(x)
    assert bool(torch.isnan(got[torch.isnan(x)]).all()), f"{tag}: a NaN input does not give a NaN"
    if bwd:
        assert bool((got[carved].float() == 0).all()), f"{tag}: x <= -89 does not give a zero"
    else:
        assert bool((M.bits(got[carved].contiguous()) == -32768).all()), f"{tag}: x <= -89 does not give -0"
    rest = ~carved
    K = M.K_SB if bwd else M.K_S
    _within(got[rest], ref[rest], M.silu_bound(ref[rest], T[rest], K), "silu backward" if bwd else "silu forward", tag,
            K * M.U24 * T[rest])


# ----------------------------------------------------------------------------------------------------------------
# adaLN modulation
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ("exact", "soft"))
@pytest.mark.parametrize("row", M.rows_of(M.MODF), ids=M.row_id)
def test_modulate_fwd_rows(row, family):
    L, tag = _L(), f"{M.row_id(row)} {family}"
    B, N, C = row.dims
    c = M.mod_case(row, family)
    ref, T = M.modf_reference(row, c)

    def once(check):
        X, RR, S, TT, Y = M.dev(c["x"]), M.dev(c["r"]), M.dev(c["s"]), M.dev(c["t"]), M.Win(B * N * C, "cuda")
        g = _guard(dict(x=X, r=RR, s=S, t=TT), dict(y=(Y, _whole(Y))))
        _run(L, lambda: L.sdmi_modulate_fwd(ptr(X.data), ptr(RR.data) if opt(row, "r", 1) else None, ptr(S.data),
                                            ptr(TT.data) if opt(row, "t", 1) else None, c["ls"], c["alpha"], ptr(Y.data), B,
                                            N, C, _stream()), row.launches, tag, check)
        _unchanged(g, tag)
        return dict(y=M.host(Y, B, N, C))

    got = _twice(once, tag)["y"]
    if family == "exact":
        _same(got, ref.float(), "y (small integers and powers of two)", tag)
    _within(got, ref, M.K_MF * M.U24 * T, f"modulate forward ({family})", tag)


@pytest.mark.parametrize("family", ("exact", "soft"))
@pytest.mark.parametrize("row", M.rows_of(M.MODB), ids=M.row_id)
def test_modulate_bwd_rows(row, family):
    L, tag = _L(), f"{M.row_id(row)} {family}"
    B, N, C = row.dims
    c = M.mod_case(row, family)
    ref = M.modb_reference(row, c)
    null = opt(row, "null")

    def once(check):
        X, DY, S, DX = M.dev(c["x"]), M.dev(c["dy"]), M.dev(c["s"]), M.Win(B * N * C, "cuda")
        DS, DT = M.Buf(B, c["ls"], torch.float32, "cuda"), M.Buf(B, c["ls"], torch.float32, "cuda")
        g = _guard(dict(x=X, dy=DY, s=S), dict(dx=(DX, [] if null == "dx" else _whole(DX)),
                                               ds=(DS, [] if null == "ds" else [("w", 0, C)]),
                                               dt=(DT, [] if null == "dt" else [("w", 0, C)])))
        _run(L, lambda: L.sdmi_modulate_bwd(ptr(X.data), ptr(DY.data), ptr(S.data), c["ls"], c["alpha"],
                                            None if null == "dx" else ptr(DX.data),
                                            None if null == "ds" else ptr(DS.window(0, C)),
                                            None if null == "dt" else ptr(DT.window(0, C)), B, N, C, _stream()),
             row.launches, tag, check)
        _unchanged(g, tag)
        return dict(dx=M.host(DX, B, N, C), ds=DS.window(0, C).cpu(), dt=DT.window(0, C).cpu())

    got = _twice(once, tag)
    if null != "dx":
        _same(got["dx"], ref["dx"], "dx (one rounded product with the fp32 alpha + s)", tag)
    for k, Tk, K in (("ds", "Ts", M.K_MS), ("dt", "Tt", M.K_MT)):
        if null == k:
            continue
        if family == "exact":
            _same(got[k], ref[k].float(), f"{k} (integer sums)", tag)
        _within(got[k], ref[k], K * M.U24 * ref[Tk], f"modulate backward {k} ({family})", tag)


# ----------------------------------------------------------------------------------------------------------------
# attention map
# ----------------------------------------------------------------------------------------------------------------
def _amap_once(L, row, c, avg, check, launches):
    B, H, N, S, d = row.dims
    tag = M.row_id(row)
    Q, K = M.dev(c["q"]), M.dev(c["k"])
    O = M.Win(B * N * S * (1 if avg else H), "cuda")
    g = _guard(dict(q=Q, k=K), dict(out=(O, _whole(O))))
    _run(L, lambda: L.sdmi_attn_map(ptr(Q.data), c["q"].shape[2], ptr(K.data), c["k"].shape[2], B, H, N, S, d, c["scaling"],
                                    avg, ptr(O.data), _stream()), launches, tag, check)
    _unchanged(g, tag)
    return dict(out=M.host(O, *((B, N, S) if avg else (B, H, N, S))))


@pytest.mark.parametrize("row", M.rows_of(M.AMAP), ids=M.row_id)
def test_attn_map_rows(row):
    L, tag = _L(), M.row_id(row)
    B, H, N, S, d = row.dims
    avg = opt(row, "avg")
    c = M.amap_case(row)
    p, T = M.amap_reference(row, c)
    got = _twice(lambda check: _amap_once(L, row, c, avg, check, row.launches), tag)["out"]
    _within(got, M.amap_out(row, p), M.amap_bound(M.amap_out(row, T)), "attention map", tag)
    if not avg:
        rows = got.double().sum(-1)
        _within(rows, torch.ones_like(rows), torch.full_like(rows, M.K_AROW * M.U24), "attention map row sums", tag)
    for family in ("equal", "peak"):
        ce = M.amap_case(row, family)
        per_head = _amap_once(L, row, ce, 0, False, None)["out"]
        if family == "equal":
            want = torch.full((B, H, N, S), 1.0) / torch.tensor(float(S))
        else:
            want = torch.zeros(B, H, N, S)
            want[..., 0] = 1.0
        _same(per_head, want, f"the per-head map of the {family} family", tag)
        if avg and H in (1, 2, 4):
            _same(_amap_once(L, row, ce, 1, False, None)["out"], want[:, 0], f"the averaged map of the {family} family", tag)
