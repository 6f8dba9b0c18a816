"""The attention kernels at the EDGES of their tile constants, against fp64 and the emulation of each split (tests/attn_emulate.py).

The generic kernel of csrc/attention.hip (every CLIP tower, every non-ViT-H geometry, every non-parity split) works in 32-query waves,
NW * 32-query workgroups (NW = 4, or 7 for windows of 129 .. 224 slots), 64-key tiles of two 32-key sub-tiles and bias tables of pitch
L | 1.  The other attention suites go deep on value distributions (tests/test_attention_peaked_gpu.py) and on win2's pair schedule
(tests/test_attention_window_pairs_gpu.py) at a handful of shapes; here the shapes sit on and around every one of those constants:
sequences of 1, 31 .. 33, 63 .. 65, 127 .. 129 and 257 tokens, token maps from 1 x 1 to 23 x 23, windows from 5 to 16 -- smaller than the
map's remainder, larger than the map, with two query blocks per window -- and win2 on maps smaller than its one window.  L = 5, 6, 7
are the sizes at which the slot -> (row, column) map of the bias needed more than the three wraps it had.

Per shape two families of tests/attn_cases.py: gauss (sigma 1) and a peak of 12 on a key of the LAST key tile, where a tail slot masked
wrongly or counted twice moves the output by O(1).  The output starts as NaN between 256 guard rows of 7.0 on either side: guards
untouched, no NaN left, and the bound of the peaked suite (attn_cases.check, no new constant) on the whole launch and again on the rows
of the last query block alone.  B = 2 and several heads: image and head offsets are non-zero.
"""
import pytest
import torch

import attn_cases as A

pytestmark = pytest.mark.gpu

GUARD = 256            # rows of 7.0 in front of and behind the output rows
CVLM_E_WORKSPACE = -3  # include/cvlm.h


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from camouflaged_vlm_amd import hip as h
    h.load()
    return h


# ---------------------------------------------------------------------------------------------------------------------------------
def guarded(M, D):
    """(2, GUARD + M + GUARD, D) fp16: 7.0 around M rows of NaN"""
    big = torch.full((2, M + 2 * GUARD, D), 7.0, dtype=torch.float16, device="cuda")
    big[:, GUARD:GUARD + M] = float("nan")
    return big


def guards_untouched(big, M):
    return bool((big[:, :GUARD] == 7.0).all()) and bool((big[:, GUARD + M:] == 7.0).all())


def device_qkv(hip, c, head_major):
    t = c.Q.t
    if head_major:
        t = torch.stack([A.to_head_major(t[i], c.B, c.S, c.Hh, c.hd) for i in range(2)])
    return hip.H2(t.cuda())


def launch(hip, c, split, head_major=True, q_rows=0, qkv=None):
    """One launch of a case into a guarded buffer -> the (2, M, D) planes of the output rows (guards checked)"""
    M = c.B * c.S
    big = guarded(M, c.D)
    out = hip.H2(big[:, GUARD:GUARD + M])                            # a row slice: each plane contiguous
    dev = lambda h: None if h is None else hip.H2(h.t.cuda())
    hip.attention(qkv if qkv is not None else device_qkv(hip, c, head_major), out, c.B, c.S, c.Hh, c.hd, mode=c.mode, grid=c.G,
                  window=c.ws, causal=c.causal, pad=dev(c.P), rel_h=dev(c.RH), rel_w=dev(c.RW), split_qk=split[0], split_pv=split[1],
                  scale=1.0, head_major=head_major, q_rows=q_rows)
    torch.cuda.synchronize()
    assert guards_untouched(big, M), f"{c.tag()} {split}: rows outside the output were written"
    return big[:, GUARD:GUARD + M].clone()


def value(planes):
    return (planes[0].float() + planes[1].float()).cpu().double()


def bounded(c, planes, split, kernel_of, splits, what="", extra=0.0, out_lo=True):
    """The bound on the whole launch and on the rows of the last query block of every sequence"""
    res = c.res(kernel_of, splits)
    got = c.layout(value(planes))
    form = A.form_of(kernel_of, split)
    tag = f"{c.tag()} {split}{what}"
    A.check(tag, got, res, form, False, extra=extra)
    A.check(tag + " last query block", got, res, form, False, rows=c.rows_of_last_block(split, out_lo), extra=extra)


def fam_ids(params, fmt):
    return [fmt(*p[:-1]) + "-" + A._fid(p[-1]) for p in params]


# ---------------------------------------------------------------------------------------------------------------------------------
MODE0 = [(S, c, f) for S in A.MODE0_S for c in (False, True) for f in A.EDGE_FAMILIES]


@pytest.mark.parametrize("S,causal,fam", MODE0, ids=fam_ids(MODE0, lambda S, c: f"S{S}-{'causal' if c else 'full'}"))
def test_plain_edges(hip, S, causal, fam):
    """Mode 0, hd 64, three heads: one key, a partial first wave, exactly one / one and a bit sub-tiles, key tiles, query blocks; token-major
    as well at S = 33 and 129."""
    c = A.edge_case(0, fam, S=S, causal=causal)
    for hm in (True, False) if S in A.MODE0_TOKEN_MAJOR else (True,):
        qkv = device_qkv(hip, c, hm)
        for sp in A.MODE0_SPLITS:
            out = launch(hip, c, sp, hm, qkv=qkv)
            bounded(c, out, sp, A.generic_of, A.MODE0_SPLITS, "" if hm else " token-major")


@pytest.mark.parametrize("split", A.MODE0_SPLITS, ids=lambda sp: f"split{sp[0]}{sp[1]}")
@pytest.mark.parametrize("q_rows", [1, 128, 129])
def test_plain_leading_query_blocks(hip, q_rows, split):
    """q_rows on causal S = 129 (two query blocks, the second holding one query): the blocks computed have the bits of the full launch,
    the rows behind them are left alone.  q_rows = 129 = S is the full launch."""
    c = A.edge_case(0, A.EDGE_FAMILIES[0], S=129, causal=True)
    qkv = device_qkv(hip, c, True)
    full = launch(hip, c, split, qkv=qkv).view(2, c.B, c.S, c.D)
    part = launch(hip, c, split, q_rows=q_rows, qkv=qkv).view(2, c.B, c.S, c.D)
    assert not torch.isnan(full).any()
    written = min(c.S, -(-q_rows // 128) * 128)
    assert torch.equal(part[:, :, :written], full[:, :, :written]), "the leading blocks differ from the full launch"
    assert bool(torch.isnan(part[:, :, written:]).all()), "rows behind the last block touched were written"


MODE1 = [(G, f) for G in A.MODE1_G for f in A.EDGE_FAMILIES]


@pytest.mark.parametrize("G,fam", MODE1, ids=fam_ids(MODE1, lambda G: f"G{G}"))
def test_global_relpos_edges(hip, G, fam):
    """Mode 1, hd 80, two heads, the generic kernel for every split: maps of 1 to 529 tokens -- L = 5, 6, 7 among them, table pitches
    L | 1 = L + 1 and L.  (2, 2) and (1, 2) run as (3, 3): the same bits."""
    c = A.edge_case(1, fam, G=G)
    for hm in (True, False) if G in A.MODE1_TOKEN_MAJOR else (True,):
        qkv = device_qkv(hip, c, hm)
        outs = {}
        for sp in A.SPLITS:
            outs[sp] = launch(hip, c, sp, hm, qkv=qkv)
            bounded(c, outs[sp], sp, A.generic_of, A.SPLITS, "" if hm else " token-major")
        assert torch.equal(outs[(2, 2)], outs[(3, 3)]) and torch.equal(outs[(1, 2)], outs[(3, 3)])


MODE2 = [(ws, G, f) for ws, G in A.MODE2_GENERIC for f in A.EDGE_FAMILIES]


@pytest.mark.parametrize("ws,G,fam", MODE2, ids=fam_ids(MODE2, lambda ws, G: f"w{ws}-G{G}"))
def test_window_relpos_edges(hip, ws, G, fam):
    """Mode 2, the generic kernel for every split (attn_cases.MODE2_GENERIC says what each shape hits)."""
    c = A.edge_case(2, fam, G=G, ws=ws)
    qkv = device_qkv(hip, c, True)
    outs = {}
    for sp in A.SPLITS:
        outs[sp] = launch(hip, c, sp, qkv=qkv)
        bounded(c, outs[sp], sp, A.generic_of, A.SPLITS)
    assert torch.equal(outs[(2, 2)], outs[(3, 3)]) and torch.equal(outs[(1, 2)], outs[(3, 3)])


W14 = [(G, f) for G in A.MODE2_W14_G for f in A.EDGE_FAMILIES]


@pytest.mark.parametrize("G,fam", W14, ids=fam_ids(W14, lambda G: f"G{G}"))
def test_window14_on_a_map_smaller_than_the_window(hip, G, fam):
    """Window 14 on 5 x 5 and 13 x 13 maps: ONE window per image, pad rows and pad columns.  win2 for (3, 3), (2, 2), (1, 2) -- its first
    run on such a map --, the generic 7-wave kernel for (3, 1), (1, 1)."""
    c = A.edge_case(2, fam, G=G, ws=14)
    qkv = device_qkv(hip, c, True)
    for sp in A.SPLITS:
        bounded(c, launch(hip, c, sp, qkv=qkv), sp, A.w14_of, A.SPLITS)


# ---------------------------------------------------------------------------------------------------------------------------------
# hi-only output (out_lo = NULL): the C ABI, cvlm_attn_args filled directly
def c_args(hip, c, qkv, out_hi, out_lo, split, rel=None, pad=None, workspace=None, scale=1.0):
    a = hip.AttnArgs()
    a.qkv_hi, a.qkv_lo = qkv.hi.data_ptr(), qkv.lo.data_ptr()
    if pad is not None:
        a.pad_hi, a.pad_lo = pad.hi.data_ptr(), pad.lo.data_ptr()
    if rel is not None:
        a.relh_hi, a.relh_lo, a.relw_hi, a.relw_lo = rel[0].hi.data_ptr(), rel[0].lo.data_ptr(), rel[1].hi.data_ptr(), rel[1].lo.data_ptr()
    a.out_hi, a.out_lo = out_hi.data_ptr(), None if out_lo is None else out_lo.data_ptr()
    a.B, a.S, a.heads, a.hd, a.mode, a.grid, a.window, a.causal = c.B, c.S, c.Hh, c.hd, c.mode, c.G, c.ws, int(c.causal)
    a.split_qk, a.split_pv, a.scale, a.qkv_layout = split[0], split[1], scale, 1
    if workspace is not None:
        a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel()
    return a


def launch_hi_only(hip, c, split, qkv):
    """-> (return code, the (M, D) hi plane); the launch gets no lo plane"""
    M = c.B * c.S
    big = guarded(M, c.D)
    dev = lambda h: hip.H2(h.t.cuda())
    keep = (dev(c.P), dev(c.RH), dev(c.RW))
    a = c_args(hip, c, qkv, big[0, GUARD:GUARD + M], None, split, rel=keep[1:], pad=keep[0])
    rc = hip.load().cvlm_attention(a, None)
    torch.cuda.synchronize()
    assert bool((big[0, :GUARD] == 7.0).all()) and bool((big[0, GUARD + M:] == 7.0).all()), "rows outside the hi plane were written"
    assert bool((big[1, :GUARD] == 7.0).all()) and bool(torch.isnan(big[1, GUARD:GUARD + M]).all()), "no lo plane was given, one was written"
    return rc, big[0, GUARD:GUARD + M].clone()


@pytest.mark.parametrize("split", A.SPLITS, ids=lambda sp: f"split{sp[0]}{sp[1]}")
def test_hi_only_output_has_the_bits_of_the_hi_plane(hip, split):
    """Generic kernel, window 8 on a 16 x 16 map: without out_lo the hi plane is the hi plane of the two-plane launch."""
    c = A.edge_case(2, A.EDGE_FAMILIES[0], G=16, ws=8)
    qkv = device_qkv(hip, c, True)
    rc, hi = launch_hi_only(hip, c, split, qkv)
    assert rc == 0
    assert torch.equal(hi, launch(hip, c, split, qkv=qkv)[0])


@pytest.mark.parametrize("G", A.MODE2_W14_G + [20])
def test_hi_only_window14_runs_the_generic_kernel(hip, G):
    """Window 14 with (3, 3) and no out_lo: win2 writes h2 only, so the launch falls to the generic 7-wave kernel -- the out_lo argument of
    hip.attention_reads_k_lo.  Against fp64 with the generic kernel's emulation, plus one fp16 rounding of the output (2^-11 relative);
    and (1, 2) there reads K's lo plane, as the predicate says."""
    c = A.edge_case(2, A.EDGE_FAMILIES[1], G=G, ws=14)
    qkv = device_qkv(hip, c, True)
    rc, hi = launch_hi_only(hip, c, (3, 3), qkv)
    assert rc == 0
    planes = torch.stack([hi, torch.zeros_like(hi)])
    bounded(c, planes, (3, 3), A.generic_of, [(3, 3)], " hi only", extra=2.0 ** -11, out_lo=False)
    assert hip.attention_reads_k_lo(2, G, 14, c.hd, 1, 2, out_lo=False)
    poisoned = hip.H2(qkv.t.clone())
    poisoned.t[1].reshape(3, -1)[1].fill_(float("nan"))               # head-major: the k third of the lo plane
    rc, hi = launch_hi_only(hip, c, (1, 2), poisoned)
    assert rc == 0 and bool(torch.isnan(hi).any()), "the predicate says K's lo plane is read, the kernel ignored it"


# ---------------------------------------------------------------------------------------------------------------------------------
# attention_g64pp.hip: launches compared with launches (no CPU reference)
G64 = [(G, sp) for G in (64, 96) for sp in ((3, 3), (1, 2))]
G64_IDS = [f"G{G}-split{sp[0]}{sp[1]}" for G, sp in G64]


class G64Case:
    """B = 2, two heads of 80 on a G x G map: Gaussian operands as in test_ops_gpu (scale hd^-0.5 at the launch)"""
    mode, ws, causal, B, Hh, hd = 1, 0, False, 2, 2, 80

    def __init__(self, hip, G, B=2, image=None):
        self.G, self.S, self.D, self.B = G, G * G, self.Hh * self.hd, B
        g = A._gen(1200 + G)
        qkv = torch.randn(2 * self.S, 3 * self.D, generator=g)
        if image is not None:
            qkv = qkv[image * self.S:(image + 1) * self.S]
        Q = hip.H2.pack(qkv)
        self.qkv = hip.H2(torch.stack([A.to_head_major(Q.t[i], B, self.S, self.Hh, self.hd) for i in range(2)]).cuda())
        self.rel = tuple(hip.H2(hip.H2.pack(torch.randn(2 * G - 1, self.hd, generator=g) * 0.2).t.cuda()) for _ in range(2))

    def tag(self):
        return f"g64pp G={self.G} B={self.B}"

    def launch(self, hip, split, workspace=None):
        M = self.B * self.S
        big = guarded(M, self.D)
        hip.attention(self.qkv, hip.H2(big[:, GUARD:GUARD + M]), self.B, self.S, self.Hh, self.hd, mode=1, grid=self.G, rel_h=self.rel[0],
                      rel_w=self.rel[1], split_qk=split[0], split_pv=split[1], head_major=True, workspace=workspace)
        torch.cuda.synchronize()
        assert guards_untouched(big, M), f"{self.tag()} {split}: rows outside the output were written"
        out = big[:, GUARD:GUARD + M].clone()
        assert not torch.isnan(out).any(), f"{self.tag()} {split}: unwritten output rows"
        return out


@pytest.mark.parametrize("G,split", G64, ids=G64_IDS)
def test_g64pp_batch_has_the_bits_of_single_images(hip, G, split):
    both = G64Case(hip, G).launch(hip, split)
    for b in range(2):
        one = G64Case(hip, G, B=1, image=b).launch(hip, split)
        assert torch.equal(both[:, b * G * G:(b + 1) * G * G], one), f"image {b} of the batch differs from its own launch"


@pytest.mark.parametrize("G,split", G64, ids=G64_IDS)
def test_g64pp_exact_workspace(hip, G, split):
    """A caller workspace of exactly attention_workspace_bytes: the bits of the implicit temporary, and not a byte written behind it."""
    c = G64Case(hip, G)
    need = hip.attention_workspace_bytes(c.B, c.S, c.Hh, c.hd, mode=1, grid=G, split_qk=split[0], split_pv=split[1])
    assert need == 2 * c.B * c.Hh * c.hd * c.S * 2                   # V^T, both planes
    buf = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device="cuda")
    ref = c.launch(hip, split)
    got = c.launch(hip, split, workspace=buf[:need])
    assert torch.equal(got, ref)
    assert bool((buf[need:] == 0x5A).all()), "bytes behind the workspace were written"
    assert not bool((buf[:need] == 0x5A).all())                       # it was the workspace that the launch used


@pytest.mark.parametrize("G,split", G64, ids=G64_IDS)
def test_g64pp_refuses_a_missing_workspace(hip, G, split):
    """NULL workspace through the C ABI: CVLM_E_WORKSPACE before any launch -- the output keeps its NaN.  One byte short: the same."""
    c = G64Case(hip, G)
    need = hip.attention_workspace_bytes(c.B, c.S, c.Hh, c.hd, mode=1, grid=G, split_qk=split[0], split_pv=split[1])
    short = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    for ws in (None, short):
        M = c.B * c.S
        big = guarded(M, c.D)
        a = c_args(hip, c, c.qkv, big[0, GUARD:GUARD + M], big[1, GUARD:GUARD + M], split, rel=c.rel, workspace=ws, scale=c.hd ** -0.5)
        rc = hip.load().cvlm_attention(a, None)
        torch.cuda.synchronize()
        assert rc == CVLM_E_WORKSPACE
        assert guards_untouched(big, M) and bool(torch.isnan(big[:, GUARD:GUARD + M]).all()), "a refused launch wrote its output"
