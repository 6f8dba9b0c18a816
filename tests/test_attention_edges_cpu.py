"""The reference side of tests/test_attention_edges_gpu.py, checked without a GPU at that suite's shapes: the window helpers of
tests/attn_cases.py where a map is smaller than its window or a multiple of it, the emulator with nothing enabled against a plain fp64
softmax at the smallest shapes, every emulated error the GPU bound multiplies -- and the slot -> (row, column) map of the generic
kernel's rel-pos bias as it was (three conditional wraps), with what that map would have cost at L = 5, 6, 7."""
import pytest
import torch

import attn_cases as A
import attn_emulate as E


def token_of(slot, wy, wx, ws, G):
    """csrc/attention.hip, token_of: the token of a window's slot, -1 for a pad slot"""
    iy, ix = divmod(slot, ws)
    y, x = wy * ws + iy, wx * ws + ix
    return -1 if y >= G or x >= G else y * G + x


@pytest.mark.parametrize("ws,G", [(8, 3), (14, 5), (14, 13), (5, 5), (8, 16), (16, 16), (7, 10), (16, 33)])
def test_window_helpers_on_small_and_exact_maps(ws, G):
    """attn_cases.windows / unwindow against the kernel's slot -> token map written out, and against the oracle's window_partition /
    window_unpartition (zero padding: a pad vector of zeros)."""
    from camouflaged_vlm_amd.hip import H2
    from oracle import cvlm_oracle as O
    Bn, Hh, hd = 2, 2, 4
    D, S = Hh * hd, G * G
    g = torch.Generator().manual_seed(ws * 100 + G)
    Q, P = H2.pack(torch.randn(Bn * S, 3 * D, generator=g)), H2.pack(torch.randn(3 * D, generator=g))
    nw = -(-G // ws)
    assert nw == (1 if G <= ws else nw) and (G % ws != 0 or nw * ws == G)
    for which in range(3):
        hi, lo = A.windows(Q, P, Bn, G, ws, Hh, hd, which)
        assert hi.shape == (Bn * nw * nw * Hh, ws * ws, hd)
        for plane, w in ((0, hi), (1, lo)):
            x = Q.t[plane].double().reshape(Bn, S, 3, Hh, hd)
            pad = P.t[plane].double().reshape(3, Hh, hd)
            w = w.reshape(Bn, nw, nw, Hh, ws * ws, hd)
            for wy in range(nw):
                for wx in range(nw):
                    for slot in range(ws * ws):
                        t = token_of(slot, wy, wx, ws, G)
                        want = pad[which].expand(Bn, Hh, hd) if t < 0 else x[:, t, which]
                        assert torch.equal(w[:, wy, wx, :, slot], want), (which, plane, wy, wx, slot)
    # unwindow: the inverse on the real tokens (pad slots have no output row)
    v = A.windows(Q, P, Bn, G, ws, Hh, hd, 2)[0]
    back = A.unwindow(v, Bn, G, ws, Hh, hd)
    assert torch.equal(back, Q.t[0].double().reshape(Bn * S, 3, D)[:, 2])
    # the oracle's partition of the same map, zero padded
    Z = H2.pack(torch.zeros(3 * D))
    x = Q.t[0].double().reshape(Bn, G, G, 3 * D)
    ow, pad_hw = O.window_partition(x, ws)                             # (Bn*nw*nw, ws, ws, 3D)
    ours = A.windows(Q, Z, Bn, G, ws, Hh, hd, 1)[0].reshape(Bn * nw * nw, Hh, ws * ws, hd)
    assert torch.equal(ours, ow.reshape(Bn * nw * nw, ws * ws, 3, Hh, hd)[:, :, 1].permute(0, 2, 1, 3))
    o = torch.randn(Bn * nw * nw, ws, ws, D, generator=g, dtype=torch.float64)
    theirs = O.window_unpartition(o, ws, pad_hw, (G, G)).reshape(Bn * S, D)
    mine = A.unwindow(o.reshape(Bn * nw * nw, ws * ws, Hh, hd).permute(0, 2, 1, 3).reshape(-1, ws * ws, hd), Bn, G, ws, Hh, hd)
    assert torch.equal(mine, theirs)


def plain_softmax_attention(c):
    """softmax(q k^T + bias) v in fp64, written without attn_emulate: (N, S, hd)"""
    q, k, v, bias, causal, scale = c.operands()
    qf, kf, vf = q[0] + q[1], k[0] + k[1], v[0] + v[1]
    s = qf @ kf.transpose(-1, -2) * scale
    if bias is not None:
        s = s + torch.stack([bias(n, torch.arange(s.shape[1])) for n in range(s.shape[0])])
    if causal:
        s = s + torch.full(s.shape[-2:], float("-inf"), dtype=torch.float64).triu_(1)
    return s.softmax(-1) @ vf


@pytest.mark.parametrize("key", [dict(mode=0, S=1), dict(mode=0, S=33, causal=True), dict(mode=1, G=7), dict(mode=2, G=7, ws=7),
                                 dict(mode=2, G=3, ws=8)], ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_emulator_without_rounding_is_the_plain_softmax(key):
    for fam in A.EDGE_FAMILIES:
        c = A.edge_case(fam=fam, **key)
        q, k, v, bias, causal, scale = c.operands()
        got = E.emulate(q, k, v, scale, bias=bias, causal=causal, f32_scores=False, online=None)
        assert float((got - plain_softmax_attention(c)).abs().max()) < 1e-12


def test_emulated_errors_of_every_edge_case_are_finite():
    """err_emulated is what the GPU bound multiplies: finite and small on every case and form, the reference without NaN, the last query
    block of every sequence not empty."""
    for key, kernel_of, splits in A.edge_cases():
        c = A.edge_case(**key)
        res = c.res(kernel_of, splits)
        ref = res["ref"]
        assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0, c.tag()
        assert 0 < res["stats"]["max_abs_score"] < 100 and res["stats"]["score_std"] == res["stats"]["score_std"], c.tag()
        for sp in splits:
            form = A.form_of(kernel_of, sp)
            assert res[form].shape == ref.shape and torch.isfinite(res[form]).all(), (c.tag(), sp)
            ee = E.relerr(res[form], ref)
            assert 0 <= ee < (2e-5 if form[:2] == ("full", "full") else 5e-3), (c.tag(), sp, ee)
            rows = c.rows_of_last_block(sp)
            assert len(rows) > 0 and int(rows.max()) < ref.shape[1], (c.tag(), sp)


# ---------------------------------------------------------------------------------------------------------------------------------
# the slot -> (row, column) map of the bias as the generic kernel had it
def three_wraps(L, b0, c):
    kh, kw = divmod(b0, L)
    kw += c
    for _ in range(3):
        if kw >= L:
            kw, kh = kw - L, kh + 1
    return min(kh, L - 1), kw


def reachable(L):
    """(b0, c) of every key slot < L * L: b0 = 64 t + 32 sub + 4 half, c = (r & 3) + 8 (r >> 2)"""
    for sub0 in range(0, L * L, 32):
        for b0 in (sub0, sub0 + 4):
            for r in range(16):
                c = (r & 3) + 8 * (r >> 2)
                if b0 + c < L * L:
                    yield b0, c


def wrong_slots(L):
    return sorted({b0 + c for b0, c in reachable(L) if three_wraps(L, b0, c) != divmod(b0 + c, L)})


def test_three_wraps_are_enough_from_L_8_only():
    """c is at most 27 and kw0 at most L - 1: three wraps reach every slot when 4 L - 1 >= L - 1 + 27.  Below: wrong (row, column) pairs
    at L = 5, 6, 7 -- none at L <= 4, whose 16 slots or fewer lie within three rows of b0 = 0 or 4."""
    assert {L: len(wrong_slots(L)) for L in range(1, 8)} == {1: 0, 2: 0, 3: 0, 4: 0, 5: 5, 6: 8, 7: 4}
    assert not any(wrong_slots(L) for L in range(8, 100))
    assert three_wraps(7, 4, 27) == (3, 10) and divmod(31, 7) == (4, 3)      # column 10 of a 7-entry row: the next query's table


@pytest.mark.parametrize("mode,ws,G", [(1, 0, 5), (1, 0, 6), (1, 0, 7), (2, 5, 5), (2, 6, 6), (2, 7, 7), (2, 7, 10)])
def test_the_three_wrap_map_fails_the_bound_at_L_5_to_7(mode, ws, G):
    """What the GPU suite's L = 5 .. 7 cases would have measured on the kernel before the fix, from the reference side alone: fp64
    attention with the bias of the wrongly mapped slots taken as the kernel took it -- Th[q][kh'] + Tw flat at q * (L | 1) + kw', which
    for kw' >= L | 1 is the table row of the NEXT query of the workgroup (an entry that is never written, or a row behind the last query,
    counts as 0: the mildest reading) -- against the true reference, in the suite's own error measure.  gauss: 0.15 to 0.44 of max |reference|,
    sixty and more times the bound of EVERY split.  peak of 12: the planted key holds nearly all the weight, so a wrong bias on other keys
    moves the output by 3e-4 to 5e-2 only -- thirty and more times the bound of (3, 3), (2, 2) and (1, 2), inside that of (3, 1) and
    (1, 1).  Every L = 5 .. 7 case of the GPU suite fails on the old map in both families."""
    L = ws or G
    ltp = L | 1
    wrong = wrong_slots(L)
    for fam in A.EDGE_FAMILIES:
        c = A.edge_case(mode, fam, G=G, ws=ws)
        q, k, v, bias, causal, scale = c.operands()
        qf = q[0] + q[1]
        N, S = qf.shape[:2]
        rh, rw = c.RH.float().double(), c.RW.float().double()
        allq = torch.arange(S)
        full = torch.stack([bias(n, allq) for n in range(N)])          # (N, S, S)
        # the per-query tables as the kernel holds them, queries in workgroup order, pitch L | 1
        kk = torch.arange(L)
        th = torch.einsum("nqc,qkc->nqk", qf, rh[(allq // L)[:, None] - kk[None, :] + L - 1])
        tw = torch.zeros(N, S + 8, ltp, dtype=torch.float64)
        tw[:, :S, :L] = torch.einsum("nqc,qkc->nqk", qf, rw[(allq % L)[:, None] - kk[None, :] + L - 1])
        twf = tw.reshape(N, -1)
        old = full.clone()
        for b0, cc in reachable(L):
            slot = b0 + cc
            if slot in wrong:
                kh, kw = three_wraps(L, b0, cc)
                old[:, :, slot] = th[:, :, kh] + twf[:, allq * ltp + kw]
        assert not torch.equal(old, full)
        res = c.res(A.generic_of, A.SPLITS)
        broken = E.emulate(q, k, v, scale, bias=old, f32_scores=False)
        if mode == 2:
            broken = A.unwindow(broken, c.B, c.G, c.ws, c.Hh, c.hd)[None]
        err = E.relerr(broken, res["ref"])
        f32 = res["stats"]["max_abs_score"] * 2.0 ** -24
        bounds = {sp: A.K_EMU * E.relerr(res[A.form_of(A.generic_of, sp)], res["ref"]) + A.FLOOR + A.C_F32 * f32 for sp in A.SPLITS}
        print(f"{c.tag()}: {len(wrong)} slots mapped wrongly, error of the old map {err:.2e}, bounds {min(bounds.values()):.1e} .. "
              f"{max(bounds.values()):.1e}")
        assert err > 10 * (max(bounds.values()) if fam[0] == "gauss" else bounds[(3, 3)]), (c.tag(), err, bounds)
