"""N2 at the edges (the metric kernels of csrc/evaltail.hip): both column passes and the row pass on either side of 64 KB of LDS of the
weighted F-measure, the vector and scalar paths of the centroid and joint-histogram kernels, mask -> uint8 and the calc_cod kernels, at
the shapes of tests/ends_cases.py against oracle/metrics_oracle.py (scipy's exact distance transform) and the numpy counters.

The weighted F-measure is held to more than its sums: d2 and Et are read back out of the workspace (csrc/evaltail.hip: near_y i32 | d2 i32
| Et f64, each [N][h][w]) and compared per pixel -- d2 with scipy's squared distances as integers, Et with |prediction - 1| at the pixel
scipy's `return_indices` names, ties included.  A wrong nearest pixel that carries a similar E passes a sum; it does not pass this."""
import numpy as np
import pytest
import torch

import ends_cases as EC
from oracle import metrics_oracle as M
from camouflaged_vlm_amd import evaltail as E

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-9        # tests/test_evaltail.py: float64 sums in another order
ET_TOL = 1e-12        # values in [0, 1] after a handful of double roundings
COD_TOL = 2e-6        # tests/test_evaltail.py::test_device_calc_cod_matches_reference: the reference sums float32 pixels


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _workspace(ws: torch.Tensor, N: int, h: int, w: int):
    px = N * h * w
    d2 = ws[4 * px:8 * px].view(torch.int32).view(N, h, w).cpu().numpy()
    et = ws[8 * px:16 * px].view(torch.float64).view(N, h, w).cpu().numpy()
    return d2, et


def _wfm_u8(pre, gt):
    from camouflaged_vlm_amd import hip
    p, g = _dev(pre), _dev(gt)
    N, h, w = pre.shape
    _, hist = E.mask_counts(p, g)
    ws = torch.zeros(hip.mask_wfm_workspace_bytes(N, h, w), dtype=torch.uint8, device="cuda")
    out = torch.full((N, 3), -1.0, dtype=torch.float64, device="cuda")
    hip.mask_wfm(p, g, hist, E._gauss49(p.device), ws, out)
    torch.cuda.synchronize()
    return (out.cpu().numpy(),) + _workspace(ws, N, h, w)


def _wfm_prob(prob, gt):
    from camouflaged_vlm_amd import hip
    p, g = _dev(prob), _dev(gt)
    N, h, w = prob.shape
    ws = torch.zeros(hip.prob_workspace_bytes(N, h, w), dtype=torch.uint8, device="cuda")
    minmax = torch.empty((N, 2), dtype=torch.float32, device="cuda")
    q = torch.empty((N, h, w), dtype=torch.uint8, device="cuda")
    hip.prob_quantise(p, minmax, q, ws)
    out = torch.full((N, 3), -1.0, dtype=torch.float64, device="cuda")
    hip.prob_wfm(p, g, minmax, E._gauss49(p.device), ws, out)
    torch.cuda.synchronize()
    return (out.cpu().numpy(),) + _workspace(ws, N, h, w)


def _check_wfm(c, n, tag, pred, fg, sums, d2, et, beta, worst):
    parts = EC.wfm_parts(pred, fg)
    if parts is None:                                                 # empty ground truth: the value is 0 (ovcos_metricer.py:56-57)
        assert sums[0] == 0 and sums[2] == 0 and E.wfm_from_sums(sums, beta) == 0.0, (c.id, n, tag)
        return
    want_sums, want_d2, want_et = parts
    ds = float(np.abs(sums - want_sums).max())
    de = float(np.abs(et - want_et).max())
    dv = abs(E.wfm_from_sums(sums, beta) - EC.wfm_value(want_sums, beta))
    worst.append((ds, de, dv))
    print(f"wfm {tag} {c.id}[{n}]: sums {ds:.3e} / {SUM_TOL:g}, Et {de:.3e} / {ET_TOL:g}, value {dv:.3e} / {SUM_TOL:g}")
    bad = np.argwhere(d2 != want_d2)
    assert len(bad) == 0, (c.id, n, tag, "d2", len(bad), bad[:4].tolist())
    bad = np.argwhere(np.abs(et - want_et) > ET_TOL)
    assert len(bad) == 0, (c.id, n, tag, "Et", len(bad), bad[:4].tolist())
    assert sums[2] == want_sums[2] and ds < SUM_TOL, (c.id, n, tag, sums.tolist(), want_sums.tolist())
    assert dv < SUM_TOL, (c.id, n, tag)


@pytest.mark.parametrize("c", EC.WFM_CASES, ids=lambda c: c.id)
def test_wfm_d2_et_and_sums(c):
    """cvlm_mask_wfm on the uint8 mask and cvlm_prob_wfm on the float map of a case.  The float entry is compared in the float64 its kernels
    compute in -- the prepared float32 prediction widened, as `(double)cod_norm(...)` -- and its value also with the reference's own float32
    pass at the calc_cod tolerance."""
    assert EC.wfm_paths(c.h, c.w) == (c.col, c.row)
    pre, prob, gt = EC.wfm_input(c)
    worst = []
    sums, d2, et = _wfm_u8(pre, gt)
    for n in range(c.N):
        pred, fg = M.prepare_data(pre[n], gt[n])
        _check_wfm(c, n, "u8", pred, fg, sums[n], d2[n], et[n], 1.0, worst)
        assert abs(E.wfm_from_sums(sums[n]) - M.wfm(pred, fg)) < SUM_TOL
    sums, d2, et = _wfm_prob(prob, gt)
    for n in range(c.N):
        pn = EC.prob_prepared(prob[n])
        fg = gt[n] > 128
        _check_wfm(c, n, "prob", pn.astype(np.float64), fg, sums[n], d2[n], et[n], 0.3, worst)
        assert abs(E.wfm_from_sums(sums[n], 0.3) - M.wfm(pn, fg, beta=0.3)) < COD_TOL


def test_wfm_refuses_sizes_past_its_limits():
    """w = 8193 and h = 16385 return CVLM_E_BADARG from both entries without launching anything: nothing is read (the buffers are a few
    bytes) and the output keeps its prefill; the limits themselves are accepted (8 x 8192 runs in test_wfm_d2_et_and_sums)"""
    from camouflaged_vlm_amd import hip
    u8 = torch.zeros(64, dtype=torch.uint8, device="cuda")
    f32 = torch.zeros(64, dtype=torch.float32, device="cuda")
    hist = torch.zeros(2048, dtype=torch.int32, device="cuda")
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.full((1, 3), -7.0, dtype=torch.float64, device="cuda")
    g = E._gauss49(u8.device)
    for h, w in EC.WFM_REFUSED + ((0, 4), (4, 0)):
        assert EC.wfm_paths(h, w) is None
        with pytest.raises(RuntimeError, match="cvlm_mask_wfm failed with code -1$"):
            hip._call("cvlm_mask_wfm", u8.data_ptr(), u8.data_ptr(), 1, h, w, hist.data_ptr(), g.data_ptr(), ws.data_ptr(), out.data_ptr())
        with pytest.raises(RuntimeError, match="cvlm_prob_wfm failed with code -1$"):
            hip._call("cvlm_prob_wfm", f32.data_ptr(), u8.data_ptr(), 1, h, w, f32.data_ptr(), g.data_ptr(), ws.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((ws == 0).all())


@pytest.mark.parametrize("c", EC.HIST_CASES, ids=lambda c: c.id)
def test_joint_hist_and_centroid_paths(c):
    """inputs as views into larger buffers filled with 255 (a read past an image counts as foreground at level 255), `stats` and `hist`
    inside prefilled buffers whose other words stay untouched"""
    from camouflaged_vlm_amd import hip
    pre, gt = EC.hist_input(c)
    nb = c.N * c.h * c.w
    views = []
    for a in (pre, gt):
        buf = torch.full((64 + 16 + nb + 64,), 255, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        v = buf[64 + c.off:64 + c.off + nb].view(c.N, c.h, c.w)
        v.copy_(_dev(a))
        views.append(v)
    p, g = views
    assert all(EC.hist_vec(c, p.data_ptr(), g.data_ptr())) == c.vec
    sbuf = torch.full((4 + 3 * c.N + 4,), -12345, dtype=torch.int64, device="cuda")
    hbuf = torch.full((16 + 2048 * c.N + 16,), -54321, dtype=torch.int32, device="cuda")
    stats, hist = sbuf[4:4 + 3 * c.N].view(c.N, 3), hbuf[16:16 + 2048 * c.N].view(c.N, 4, 2, 256)
    hip.mask_joint_hist(p, g, stats, hist)
    torch.cuda.synchronize()
    for n in range(c.N):
        ws, wh = EC.counts_numpy(pre[n], gt[n])
        assert np.array_equal(stats[n].cpu().numpy(), ws), (c.id, n, stats[n].tolist(), ws.tolist())
        assert np.array_equal(hist[n].cpu().numpy().astype(np.int64), wh), (c.id, n)
    assert bool((sbuf[:4] == -12345).all()) and bool((sbuf[4 + 3 * c.N:] == -12345).all())
    assert bool((hbuf[:16] == -54321).all()) and bool((hbuf[16 + 2048 * c.N:] == -54321).all())


@pytest.mark.parametrize("src", EC.MASK_SOURCES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mask_to_u8_exact_on_exact_sigmoids(src):
    """logits from {-40, 0, +40}: the sigmoids are exactly 1, exactly 0.5 and below 1e-17 whatever the last bit of exp, and every later
    operation is the oracle's fp32 product and sum -- no pixel is excused"""
    from camouflaged_vlm_amd import hip
    lg = EC.mask_logits(src)
    dev = _dev(lg)
    for dst in EC.MASK_TARGETS:
        h, w = dst or src
        nb = EC.MASK_N * h * w
        buf = torch.full((64 + nb + 64,), EC.SENTINEL, dtype=torch.uint8, device="cuda")
        out = buf[64:64 + nb].view(EC.MASK_N, h, w)
        hip.mask_to_u8(dev, h, w, out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for n in range(EC.MASK_N):
            want = M.mask_to_u8(lg[n], h, w)
            assert np.array_equal(got[n], want), (src, dst, n, int((got[n] != want).sum()))
        assert bool((buf[:64] == EC.SENTINEL).all()) and bool((buf[64 + nb:] == EC.SENTINEL).all())
        assert np.array_equal(E.mask_to_u8(dev[:, None], h, w).cpu().numpy(), got)


@pytest.mark.parametrize("name", EC.COD_CASES)
def test_calc_cod_kernels_at_the_edges(name):
    """cod_counts / DeviceCod against metrics_oracle.calc_cod; the integer parts (levels, counters) of every image equal numpy's, so one
    image's min / max cannot have reached another's"""
    prob, gt = EC.cod_input(name)
    g = _dev((gt[:, 0] * 255).astype(np.uint8))
    c = E.DeviceCod()
    c.step(_dev(prob), g)
    got = c.result()
    for key, want in zip(("sm", "em", "wfm", "mae"), M.calc_cod(prob, gt)):
        assert abs(got[key] - want) < COD_TOL, (name, key, got[key], want)
    stats, hist, mom, wsum = (t.cpu().numpy() for t in E.cod_counts(_dev(prob), g))
    for k in range(len(prob)):
        gk = (gt[k, 0] * 255).astype(np.uint8)
        ws, wh, wm, pn, fg = EC.cod_counts_numpy(prob[k, 0], gk)
        assert np.array_equal(stats[k], ws) and np.array_equal(hist[k].astype(np.int64), wh), (name, k)
        assert np.allclose(mom[k], wm, rtol=1e-12, atol=1e-9), (name, k)
        want_sums = EC.wfm_parts(pn.astype(np.float64), fg)[0]
        assert np.abs(wsum[k] - want_sums).max() < SUM_TOL, (name, k, wsum[k].tolist(), want_sums.tolist())
        one = E.DeviceCod()
        one.step(_dev(prob[k:k + 1]), g[k:k + 1])
        for key, want in zip(("sm", "em", "wfm", "mae"), M.calc_cod(prob[k:k + 1], gt[k:k + 1])):
            assert abs(one.result()[key] - want) < COD_TOL, (name, k, key)
