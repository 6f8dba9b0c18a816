"""What the attention suites share (tests/test_attention_peaked_gpu.py, tests/test_attention_edges_gpu.py and, for the reference side
alone, tests/test_attention_edges_cpu.py): operand families built from packed planes, the fp64 side of a case with the emulation of
each split's rounding points (tests/attn_emulate.py), the bound, and the list of edge shapes.  Importable without a GPU.

Bound per case: err_kernel <= K_EMU * err_emulated + FLOOR + C_F32 * max|s| * 2^-24 (relative to max |reference|), with the emulation of
THAT split on the same operands; and, for the lossy ViT-H kernels, err_kernel > LOSSY_MIN * err_emulated (a silent fall-back to (3, 3)
fails).
"""
import math

import torch

import attn_emulate as E

K_EMU = 2.5         # kernel error / emulated error: the emulation takes the rounding points, not the fp32 summation order
FLOOR = 2e-6        # relative: fp32 scores and exponentials of |s| up to ~400 (the +6-per-tile ramp on 4096 keys)
LOSSY_MIN = 0.2     # a lossy kernel's error is at least this fraction of its emulation's
# fp32 online softmax: the output accumulators, rescale factors and fp32 products of the kernels carry errors of |s| * 2^-24 grade that the
# emulation does not take; this many units of max|s| * 2^-24 are allowed on top (measured: at most 4.1, the 96 x 96 map with a peak of 12).
# Measured kernel / emulation on the lossy ViT-H kernels: 0.79-1.08; on the generic (3, 1) / (1, 1): up to 1.48.
C_F32 = 8.0
SPLITS = [(3, 3), (2, 2), (1, 2), (3, 1), (1, 1)]


# ---------------------------------------------------------------------------------------------------------------------------------
# operands
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def family_terms(fam, nq, nk, window_local=None):
    """(q coordinate per query, k coordinate per key) of the planted / ramp families; window_local maps token -> key index in its window."""
    kind = fam[0]
    jq = torch.arange(nq) if window_local is None else window_local
    jk = torch.arange(nk) if window_local is None else window_local
    tile = (jk // 64).double()
    if kind == "ramp":
        how = fam[1]
        if how == "slow":
            r, cq = tile * 1.0, torch.ones(nq)
        elif how == "fast":
            r, cq = tile * 6.0, torch.ones(nq)
        elif how == "half":
            r, cq = tile * 6.0, ((jq % 32) < 16).double()
        else:                                                            # "desc"
            r, cq = (tile.max() - tile) * 1.0, torch.ones(nq)
        return cq.double(), r
    if kind == "peak":
        d, where = fam[1], fam[2]
        r = torch.zeros(nk, dtype=torch.float64)
        if where == "first":
            r[jk == 5] = d
        elif where == "last":
            r[jk == int(jk.max()) - 2] = d
        return torch.ones(nq, dtype=torch.float64), r
    return None


def sigma_of(fam):
    return fam[1] if fam[0] == "gauss" else 1.0


def make_qkv(fam, B, S, Hh, hd, seed, window=0, G=0):
    """Token-major fp32 qkv [B*S][3*Hh*hd] with the family's score structure (scale = 1: q carries it, as in the engine) and the
    rel-pos table std that makes the bias ~0.3 sigma.  Coordinate 0 of every head carries the planted / ramp term."""
    g = _gen(seed)
    sig = sigma_of(fam)
    a = math.sqrt(sig) / hd ** 0.25
    x = torch.randn(B * S, 3, Hh, hd, generator=g, dtype=torch.float64)
    x[:, 0] *= a
    x[:, 1] *= a
    wl = None
    if window:
        ty, tx = torch.arange(S) // G, torch.arange(S) % G
        wl = (ty % window) * window + (tx % window)
    terms = family_terms(fam, S, S, wl)
    if terms is not None:
        cq, r = terms
        x[:, 0, :, 0] = cq.repeat(B)[:, None]
        x[:, 1, :, 0] = r.repeat(B)[:, None]
    rstd = 0.3 * sig / (math.sqrt(2.0) * a * math.sqrt(hd))
    return x.reshape(B * S, 3 * Hh * hd).float(), rstd


def to_head_major(t, Bn, S, Hh, hd):
    return t.reshape(Bn, S, 3, Hh, hd).permute(2, 0, 3, 1, 4).contiguous().reshape(Bn * S, 3 * Hh * hd)


def planes_bhsd(P, which, Bn, S, Hh, hd):
    """(hi, lo) fp64 of q / k / v (which = 0 / 1 / 2) as (B*Hh, S, hd) from token-major planes."""
    return tuple(P.t[i].double().cpu().reshape(Bn, S, 3, Hh, hd)[:, :, which].permute(0, 2, 1, 3).reshape(Bn * Hh, S, hd) for i in (0, 1))


def relpos_rows(qf, RH, RW, L):
    """Callable bias rows of image_encoder.py:589-625 for queries qf (N, L*L, hd) fp64 and tables (2L-1, hd) fp64."""
    def rows(n, r):
        qh, qw = r // L, r % L
        kk = torch.arange(L)
        Rh = RH[(qh[:, None] - kk[None, :] + L - 1)]                  # (rows, L, hd)
        Rw = RW[(qw[:, None] - kk[None, :] + L - 1)]
        th = torch.einsum("rc,rkc->rk", qf[n, r], Rh)
        tw = torch.einsum("rc,rkc->rk", qf[n, r], Rw)
        return (th[:, :, None] + tw[:, None, :]).reshape(len(r), L * L)
    return rows


def windows(planes, pad_planes, Bn, G, ws, Hh, hd, which):
    """(hi, lo) of q / k / v per window, pad tokens = the pad vector: (Bn*nw*nw*Hh, ws*ws, hd)."""
    Gp = -(-G // ws) * ws
    nw = Gp // ws
    out = []
    for i in (0, 1):
        x = planes.t[i].double().cpu().reshape(Bn, G, G, 3 * Hh * hd)
        xp = pad_planes.t[i].double().cpu().expand(Bn, Gp, Gp, 3 * Hh * hd).clone()
        xp[:, :G, :G] = x
        w = xp.reshape(Bn, nw, ws, nw, ws, 3, Hh, hd)[:, :, :, :, :, which].permute(0, 1, 3, 5, 2, 4, 6)
        out.append(w.reshape(Bn * nw * nw * Hh, ws * ws, hd))
    return tuple(out)


def unwindow(o, Bn, G, ws, Hh, hd):
    Gp = -(-G // ws) * ws
    nw = Gp // ws
    o = o.reshape(Bn, nw, nw, Hh, ws, ws, hd).permute(0, 1, 4, 2, 5, 3, 6).reshape(Bn, Gp, Gp, Hh * hd)
    return o[:, :G, :G].reshape(Bn * G * G, Hh * hd)


# ---------------------------------------------------------------------------------------------------------------------------------
# the fp64 side of a case, computed once per (dispatch geometry, family) and shared by every split
_CPU = {}


def cpu_side(key, build):
    if key not in _CPU:
        _CPU[key] = build()
    return _CPU[key]


def sampled_rows(S):
    """Queries the fp64 side computes: all of them up to 2048; beyond, every 4th block of 256 (whole workgroups of every kernel, both
    halves of every 32-query group) -- the CPU cost of a 96 x 96 map drops 9x, every kernel row is still checked for being written."""
    r = torch.arange(S)
    return r if S <= 2048 else r[(r // 256) % (4 if S <= 4096 else 9) == 0]


def emulations(ops, kernel_of, splits, rows=None):
    """Reference (no rounding at all) + the emulation of every split, on the same operands.  kernel_of(split) -> (family, online softmax
    of that kernel: (key tile, tau))."""
    q, k, v, bias, causal, scale = ops
    st = {}
    res = {"ref": E.emulate(q, k, v, scale, bias=bias, causal=causal, f32_scores=False, rows=rows, stats=st), "stats": st}
    for sp in splits:
        fam, online = kernel_of(sp)
        form = E.rounding(fam, sp) + (online,)
        if form not in res:
            res[form] = E.emulate(q, k, v, scale, bias=bias, causal=causal, qk=form[0], pv=form[1], online=online, rows=rows)
    return res


def form_of(kernel_of, sp):
    fam, online = kernel_of(sp)
    return E.rounding(fam, sp) + (online,)


# online softmax of each kernel: key tile and how far the maximum must move before the reference point does
GENERIC64 = (E.GENERIC, (64, 5.0))                   # csrc/attention.hip: 64-key tiles, lazy (TAU = 5)
WIN2 = (E.VITH, (32, 5.0))                           # attention_win2.hip: 32-key tiles, lazy
G64PAIR = (E.VITH, (64, 0.0))                        # attention_g64pp.hip, 64 x 64 map: a key row (64 keys) per phase, every new maximum
G96PP = (E.VITH, (32, 0.0))                          # attention_g64pp.hip, 96 x 96 map: 32-key tiles


def check(tag, got, res, form, lossy_vith, rows=None, extra=0.0):
    """extra: a rounding the case adds on top of the kernel's own (relative to max |reference|), e.g. an output kept as one fp16."""
    ref, emu = res["ref"], res[form]
    assert not torch.isnan(got).any(), f"{tag}: unwritten output rows"
    if rows is not None:
        got, ref, emu = got[:, rows], ref[:, rows], emu[:, rows]
    ek, ee = E.relerr(got, ref), E.relerr(emu, ref)
    st = res["stats"]
    print(f"{tag}: score std {st['score_std']:.2f} max|s| {st['max_abs_score']:.1f} H/lnN {st['entropy_ratio']:.3f} | kernel {ek:.2e} "
          f"emulated {ee:.2e} ratio {ek / max(ee, 1e-30):.2f}")
    f32 = st["max_abs_score"] * 2.0 ** -24
    print(f"    units of max|s| 2^-24 beyond K_EMU * emulated + FLOOR: {(ek - K_EMU * ee - FLOOR - extra) / f32:.2f}")
    assert ek <= K_EMU * ee + FLOOR + C_F32 * f32 + extra, (tag, ek, ee)
    if lossy_vith:                                   # not better than it can be: the lossy kernel ran, not (3, 3)
        assert ek > LOSSY_MIN * ee and (ek > 5e-6 or ee < 2.5e-5), (tag, ek, ee)


def _fid(f):
    return "-".join(str(x) for x in f)


# ---------------------------------------------------------------------------------------------------------------------------------
# Edge shapes of the generic kernel's tile constants (csrc/attention.hip: 32-query waves, NW * 32-query blocks with NW = 4 or 7, 64-key
# tiles with 32-key sub-tiles, table pitch L | 1) and of win2 on a map smaller than its window.  Two families per shape: in the second
# the weight sits on a key of the last tile, so a tail slot masked wrongly or counted twice moves the output by O(1).
EDGE_FAMILIES = [("gauss", 1), ("peak", 12, "last")]
EDGE_B = 2                                           # image and head offsets are non-zero
MODE0_S = [1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 257]
MODE0_HEADS, MODE0_HD, MODE0_SPLITS = 3, 64, [(3, 3), (3, 1), (1, 1)]
MODE0_TOKEN_MAJOR = (33, 129)
MODE1_G = [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 16, 23]
MODE1_TOKEN_MAJOR = (7, 11)
REL_HEADS, REL_HD = 2, 80
# (window, grid): (5,5) (6,6) (7,7) (7,10) the slot -> (row, column) map below L = 8; (8,16) no pad; (8,3) one mostly-pad window; (11,20) a
# partial fourth wave; (13,20) the 7-wave form with its seventh wave idle; (15,20) / (16,16) two query blocks per window with a ragged / an
# exact last key tile; (16,33) that with a one-token remainder
MODE2_GENERIC = [(5, 5), (6, 6), (7, 7), (7, 10), (8, 16), (8, 3), (11, 20), (13, 20), (15, 20), (16, 16), (16, 33)]
MODE2_W14_G = [5, 13]                                # window 14 on a map smaller than one window: win2 for the parity splits, generic otherwise
W14_WIN2_SPLITS, W14_GENERIC_SPLITS = [(3, 3), (2, 2), (1, 2)], [(3, 1), (1, 1)]


def generic_of(sp):
    return GENERIC64


def w14_of(sp):
    return WIN2 if sp in W14_WIN2_SPLITS else GENERIC64


def query_block(mode, ws, split=(3, 3), out_lo=True):
    """Queries per workgroup of the kernel that runs (cvlm_attention's dispatch restated): 128 or, for windows of 129 .. 224 slots, 224;
    win2 holds a whole 14 x 14 window."""
    if mode == 2 and ws == 14 and split in W14_WIN2_SPLITS and out_lo:
        return 224
    return 224 if mode == 2 and 128 < ws * ws <= 224 else 128


def last_block_rows(mode, S, G=0, ws=0, split=(3, 3), out_lo=True):
    """Token indices (within an image) of the queries of the LAST query block of their sequence."""
    if mode != 2:
        return torch.arange(((S - 1) // 128) * 128, S)
    qb = query_block(mode, ws, split, out_lo)
    t = torch.arange(G * G)
    wl = ((t // G) % ws) * ws + (t % G) % ws
    return t[wl >= ((ws * ws - 1) // qb) * qb]


class Case:
    """Host side of one shape and family: packed planes (hip.H2 on the CPU) and, on request, the fp64 reference with the emulations of
    the splits asked for (kept: one computation per case and process)."""

    def __init__(self, mode, fam, S, Hh, hd, causal=False, G=0, ws=0):
        from camouflaged_vlm_amd.hip import H2
        self.mode, self.fam, self.S, self.Hh, self.hd, self.causal, self.G, self.ws = mode, fam, S, Hh, hd, causal, G, ws
        self.B, self.D = EDGE_B, Hh * hd
        L = ws or G
        qkv, rstd = make_qkv(fam, self.B, S, Hh, hd, seed=900 + 7 * S + 3 * ws + mode, window=ws, G=G)
        self.Q = H2.pack(qkv)
        self.P = self.RH = self.RW = None
        if mode:
            g = _gen(950 + G + 5 * ws)
            if mode == 2:
                pad = torch.randn(3, Hh, hd, generator=g, dtype=torch.float64) / hd ** 0.25
                if fam[0] == "peak":
                    pad[0, :, 0], pad[1, :, 0] = 1.0, 0.0
                self.P = H2.pack(pad.reshape(3 * self.D).float())
            self.RH = H2.pack(torch.randn(2 * L - 1, hd, generator=g) * rstd)
            self.RW = H2.pack(torch.randn(2 * L - 1, hd, generator=g) * rstd)
        self._res = {}

    def tag(self):
        shape = {0: f"S={self.S} causal={self.causal}", 1: f"G={self.G}", 2: f"w={self.ws} G={self.G}"}[self.mode]
        return f"mode {self.mode} {shape} {_fid(self.fam)}"

    def operands(self):
        """(q, k, v, bias rows, causal, scale) in the sequences the kernels run: images, or windows with their pad tokens."""
        B, S, Hh, hd = self.B, self.S, self.Hh, self.hd
        if self.mode == 2:
            q, k, v = (windows(self.Q, self.P, B, self.G, self.ws, Hh, hd, w) for w in range(3))
        else:
            q, k, v = (planes_bhsd(self.Q, w, B, S, Hh, hd) for w in range(3))
        bias = None
        if self.mode:
            bias = relpos_rows(q[0] + q[1], self.RH.float().double(), self.RW.float().double(), self.ws or self.G)
        return q, k, v, bias, self.causal, 1.0

    def res(self, kernel_of, splits):
        """{"ref", "stats", form: emulation} in the layout of the output: (B*Hh, S, hd) for modes 0 / 1, (1, B*S, D) for mode 2."""
        missing = [sp for sp in splits if form_of(kernel_of, sp) not in self._res]
        if missing:                                                   # forms asked for later join the first ones (the reference comes out the same)
            new = emulations(self.operands(), kernel_of, missing)
            if self.mode == 2:
                new = {k: (v if k == "stats" else unwindow(v, self.B, self.G, self.ws, self.Hh, self.hd)[None]) for k, v in new.items()}
            self._res = {**new, **self._res}
        return self._res

    def layout(self, out):
        """fp64 (tokens, D) output -> the layout of res()."""
        if self.mode == 2:
            return out[None]
        return out.reshape(self.B, self.S, self.Hh, self.hd).permute(0, 2, 1, 3).reshape(self.B * self.Hh, self.S, self.hd)

    def rows_of_last_block(self, split=(3, 3), out_lo=True):
        r = last_block_rows(self.mode, self.S, self.G, self.ws, split, out_lo)
        if self.mode == 2:                                            # the (1, B*S, D) layout: every image's rows
            r = torch.cat([r + b * self.S for b in range(self.B)])
        return r


_CASES = {}


def edge_case(mode, fam, S=0, causal=False, G=0, ws=0):
    """The case of a shape, built once per process."""
    key = (mode, fam, S, causal, G, ws)
    if key not in _CASES:
        if mode == 0:
            _CASES[key] = Case(0, fam, S, MODE0_HEADS, MODE0_HD, causal=causal)
        else:
            _CASES[key] = Case(mode, fam, G * G, REL_HEADS, REL_HD, G=G, ws=ws)
    return _CASES[key]


def edge_cases():
    """Every (case key, kernel_of, splits) of tests/test_attention_edges_gpu.py: what the GPU suite launches and the CPU suite emulates."""
    out = []
    for fam in EDGE_FAMILIES:
        out += [(dict(mode=0, fam=fam, S=S, causal=c), generic_of, MODE0_SPLITS) for S in MODE0_S for c in (False, True)]
        out += [(dict(mode=1, fam=fam, G=G), generic_of, SPLITS) for G in MODE1_G]
        out += [(dict(mode=2, fam=fam, G=G, ws=ws), generic_of, SPLITS) for ws, G in MODE2_GENERIC]
        out += [(dict(mode=2, fam=fam, G=G, ws=14), w14_of, SPLITS) for G in MODE2_W14_G]
    return out
