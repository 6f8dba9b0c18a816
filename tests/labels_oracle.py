"""Oracle of label maps (include/cvlm.h: cvlm_label_*): the values are oracle/metrics_oracle.py's own
`resize_linear_f32(sigmoid_f32(.))` -- imported, not copied, as tests/sized_oracle.py does --, then the published per-pixel argmax and
per-query loop of Mask2Former's panoptic_inference and mmseg's intersect_and_union, each written out plainly in numpy loop for loop;
an fp64 restatement of the scores that says where the best and the second-best score of a pixel lie within rounding of each other; the
runner of the entries into sentinel-guarded outputs; the inputs of the tests.  Importable without a GPU.

The one inexact comparison is `winner` on smooth logits: device expf, host expf and numpy differ in the last bits of v.  MEASURED is
the largest |s (float32 oracle) - s (fp64 restatement)| over the smooth inputs below (`smooth_cases`; tests/test_labels_cpu.py
re-measures it and holds it under this figure), MARGIN five times that, as §19 took its 2.5e-4."""
import numpy as np
import torch

from oracle import metrics_oracle as M
import sized_oracle as SO

MEASURED = 1.7e-7             # largest |fp32 - fp64| of s over smooth_cases(): 1.69e-7 measured, weights up to 1.0 (test_labels_cpu.py)
MARGIN = 5 * MEASURED         # a pixel is left out of the winner comparison where best - second best (fp64) <= MARGIN.  Absolute: the
#                               rounding error of s grows with the weight, so it holds for |weight| <= 1 only (`compare` refuses others)
GUARD = 16                    # sentinel pixels before and behind the maps
FILL_F32, FILL_I16, FILL_I32 = -123.0, -21846, -7


# ---- definition -------------------------------------------------------------------------------------------------------------------------
def values(logits: np.ndarray, h: int, w: int) -> np.ndarray:
    """f32 (K, Hs, Ws) -> f32 (K, h, w): the reference's float mask of every hypothesis."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([M.resize_linear_f32(M.sigmoid_f32(p), h, w) for p in logits]).astype(np.float32)


def bits_of(v: np.ndarray, level: int) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return (v * np.float32(255)) >= np.float32(level)


def scores_f64(logits: np.ndarray, h: int, w: int, weights) -> np.ndarray:
    """s in float64 from the same taps and the same float32 weights (K, h, w); NaN where a hypothesis takes no part."""
    K = logits.shape[0]
    wts = np.ones(K, np.float32) if weights is None else np.asarray(weights, np.float32)
    with np.errstate(invalid="ignore"):
        return np.stack([SO.levels_f64(logits[k], h, w) / 255.0 * np.float64(wts[k]) for k in range(K)])


def winner_of(v: np.ndarray, weights) -> tuple:
    """The per-pixel argmax in increasing k -> (winner int16 (h, w), score f32 (h, w)).  A hypothesis takes part iff neither its weight
    nor its value is NaN; the first to take part is taken, a later one only if its score is strictly larger."""
    K, h, w = v.shape
    wts = np.ones(K, np.float32) if weights is None else np.asarray(weights, np.float32)
    win = np.full((h, w), -1, np.int16)
    best = np.zeros((h, w), np.float32)
    for k in range(K):
        if np.isnan(wts[k]):
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            s = (wts[k] * v[k]).astype(np.float32)
            take = ~np.isnan(v[k]) & ((win < 0) | (s > best))
        win[take] = k
        best[take] = s[take]
    return win, best


def panoptic(winner: np.ndarray, bits: np.ndarray, overlap_threshold: float = 0.8) -> dict:
    """The published loop over the queries of one image on a given argmax map and given binary masks (K, h, w)."""
    K = bits.shape[0]
    segment = np.full(winner.shape, -1, np.int16)
    orig, won, kept_area = np.zeros(K, np.int32), np.zeros(K, np.int32), np.zeros(K, np.int32)
    ids = np.zeros(K, np.int32)
    current = 0
    for k in range(K):
        mine = winner == k
        mask_area = int(mine.sum())
        original_area = int(bits[k].sum())
        mask = mine & bits[k]
        orig[k], won[k], kept_area[k] = original_area, mask_area, int(mask.sum())
        if mask_area > 0 and original_area > 0 and mask.sum() > 0:
            if mask_area / original_area < overlap_threshold:
                continue
            current += 1
            ids[k] = current
            segment[mask] = k
    return dict(segment=segment, orig_area=orig, won_area=won, kept_area=kept_area, segment_id=ids, n_segments=current)


def intersect_and_union(pred, gt, C: int, ignore_index: int = 255, reduce_zero_label: bool = False) -> np.ndarray:
    """-> int64 (3, C) = (area_intersect, area_pred_label, area_label) of flat maps.  The one deviation from np.histogram(bins =
    arange(C + 1)): a value outside [0, C - 1] is counted nowhere (the closed last bin would count the value C in class C - 1)."""
    pred = np.asarray(pred).astype(np.int64).reshape(-1)
    gt = np.asarray(gt).astype(np.int64).reshape(-1)
    if reduce_zero_label:
        gt = gt.copy()
        gt[gt == 0] = 255
        gt = gt - 1
        gt[gt == 254] = 255
    keep = gt != ignore_index
    pred, gt = pred[keep], gt[keep]
    count = lambda a: np.bincount(a[(a >= 0) & (a < C)], minlength=C).astype(np.int64)
    return np.stack([count(pred[pred == gt]), count(pred), count(gt)])


def label_maps(logits: np.ndarray, sizes, weights=None, level: int = 128, overlap_threshold: float = 0.8) -> list:
    """logits f32 (B, K, Hs, Ws) -> per image the dict of `panoptic` plus winner and score."""
    out = []
    B, K = logits.shape[:2]
    wts = None if weights is None else np.asarray(weights, np.float32).reshape(B, K)
    for b, (h, w) in enumerate(sizes):
        v = values(logits[b], h, w)
        win, score = winner_of(v, None if wts is None else wts[b])
        res = panoptic(win, bits_of(v, level), overlap_threshold)
        res.update(winner=win, score=score)
        out.append(res)
    return out


def near_ties(logits: np.ndarray, h: int, w: int, weights, margin: float = MARGIN) -> np.ndarray:
    """bool (h, w): the pixels whose best and second-best fp64 score lie within `margin` (one taking part alone is never near)."""
    s = scores_f64(logits, h, w, weights)
    s = np.where(np.isnan(s), -np.inf, s)
    if s.shape[0] < 2:
        return np.zeros((h, w), bool)
    top = np.sort(s, axis=0)[-2:]
    with np.errstate(invalid="ignore"):
        return np.isfinite(top[0]) & (top[1] - top[0] <= margin)


# ---- runner -----------------------------------------------------------------------------------------------------------------------------
def tables(sizes):
    dims = np.asarray(sizes, dtype=np.int32).reshape(-1, 2)
    pix = dims[:, 0].astype(np.int64) * dims[:, 1].astype(np.int64)
    off = np.zeros(len(sizes) + 1, np.int64)
    off[1:] = np.cumsum(pix)
    return dims, off, int(pix.max())


class State:
    """Sentinel-filled outputs on `dev`: the three maps are views GUARD pixels inside larger tensors, the integer tables views one
    entry inside theirs."""

    def __init__(self, sizes, K: int, dev="cpu", n_pix=None):
        from camouflaged_vlm_amd import hip
        self.hip, self.dev, self.sizes, self.K, self.B = hip, dev, list(sizes), K, len(sizes)
        self.host = dev == "cpu"
        dims, off, self.max_pixels = tables(sizes)
        self.n = int(off[-1]) if n_pix is None else n_pix
        self.host_off = off
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.dims, self.off = t(dims), t(off)
        P, B, G = self.B * K, self.B, GUARD
        self.raw = dict(score=torch.full((self.n + 2 * G,), FILL_F32, dtype=torch.float32, device=dev),
                        winner=torch.full((self.n + 2 * G,), FILL_I16, dtype=torch.int16, device=dev),
                        segment=torch.full((self.n + 2 * G,), FILL_I16, dtype=torch.int16, device=dev),
                        areas=torch.full((3 * P + 2,), FILL_I32, dtype=torch.int32, device=dev),
                        segment_id=torch.full((P + 2,), FILL_I32, dtype=torch.int32, device=dev),
                        n_segments=torch.full((B + 2,), FILL_I32, dtype=torch.int32, device=dev),
                        status=torch.full((3,), FILL_I32, dtype=torch.int32, device=dev))
        r = self.raw
        self.score, self.winner, self.segment = (r[n][G:G + self.n] for n in ("score", "winner", "segment"))
        self.areas, self.segment_id = r["areas"][1:1 + 3 * P].view(3, P), r["segment_id"][1:1 + P]
        self.n_segments, self.status = r["n_segments"][1:1 + B], r["status"][1:2]

    def init(self):
        self.hip.label_init(self.score, self.winner, self.segment, self.areas, self.segment_id, self.n_segments, self.status, self.B, self.K,
                            host=self.host)

    def accumulate(self, planes, p0: int, weights=None, level: int = 128, dims=None, off=None):
        t = planes if isinstance(planes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(planes)).to(self.dev)
        wts = None if weights is None else torch.from_numpy(np.asarray(weights, np.float32).reshape(-1).copy()).to(self.dev)
        self.hip.label_accumulate(t, p0, self.B, self.K, self.dims if dims is None else dims, self.off if off is None else off, wts, level,
                                  self.score, self.winner, self.segment, self.max_pixels, self.areas, self.status, host=self.host)

    def finish(self, overlap_threshold: float = 0.8, dims=None, off=None):
        self.hip.label_finish(self.B, self.K, self.dims if dims is None else dims, self.off if off is None else off, overlap_threshold,
                              self.winner, self.segment, self.max_pixels, self.areas, self.segment_id, self.n_segments, self.status,
                              host=self.host)

    def lookup(self, which: str, table, void: int):
        out = torch.full((self.n + 2 * GUARD,), FILL_I32, dtype=torch.int32, device=self.dev)
        tab = torch.from_numpy(np.asarray(table, np.int32).reshape(-1).copy()).to(self.dev)
        self.hip.label_lookup(getattr(self, which), self.B, self.K, self.dims, self.off, self.max_pixels, tab, void, out[GUARD:GUARD + self.n],
                              self.status, host=self.host)
        got = out.cpu().numpy()
        assert (got[:GUARD] == FILL_I32).all() and (got[GUARD + self.n:] == FILL_I32).all(), "lookup wrote outside its map"
        return got[GUARD:GUARD + self.n]

    def read(self) -> dict:
        """Everything on the host, the guard bands checked -> per-image maps and (B, K) tables."""
        if not self.host:
            torch.cuda.synchronize()
        G, n, P, B, K = GUARD, self.n, self.B * self.K, self.B, self.K
        raw = {k: v.cpu().numpy().copy() for k, v in self.raw.items()}          # a copy: on the host .cpu() is the state itself
        for name, fill in (("score", np.float32(FILL_F32)), ("winner", FILL_I16), ("segment", FILL_I16)):
            assert (raw[name][:G] == fill).all() and (raw[name][G + n:] == fill).all(), f"{name}: a guard pixel was overwritten"
        for name, m in (("areas", 3 * P), ("segment_id", P), ("n_segments", B), ("status", 1)):
            assert raw[name][0] == FILL_I32 and raw[name][1 + m] == FILL_I32, f"{name}: a guard entry was overwritten"
        pix = [h * w for h, w in self.sizes]                          # an image whose h * w pixels from its offset on leave the maps: None
        cut = lambda a: [a[G + self.host_off[b]:G + self.host_off[b] + pix[b]].reshape(self.sizes[b])
                         if 0 <= self.host_off[b] and self.host_off[b] + pix[b] <= n else None for b in range(B)]
        areas = raw["areas"][1:1 + 3 * P].reshape(3, B, K)
        return dict(score=cut(raw["score"]), winner=cut(raw["winner"]), segment=cut(raw["segment"]), orig_area=areas[0], won_area=areas[1],
                    kept_area=areas[2], segment_id=raw["segment_id"][1:1 + P].reshape(B, K), n_segments=raw["n_segments"][1:1 + B],
                    status=int(raw["status"][1]))


def run(logits: np.ndarray, sizes, weights=None, level: int = 128, overlap_threshold: float = 0.8, dev="cpu", cuts=None, state=None) -> dict:
    """init, accumulate over the planes cut at `cuts` (plane indices; None: one call), finish -> State.read()."""
    B, K, Hs, Ws = logits.shape
    st = State(sizes, K, dev) if state is None else state
    planes = torch.from_numpy(np.ascontiguousarray(logits.reshape(B * K, Hs, Ws))).to(dev)
    st.init()
    edges = [0] + list(cuts or []) + [B * K]
    for a, b in zip(edges[:-1], edges[1:]):
        st.accumulate(planes[a:b], a, weights, level)
    st.finish(overlap_threshold)
    return st.read()


def check_integer_stages(got: dict, bits: list, overlap_threshold: float = 0.8) -> None:
    """Everything behind the argmax, exactly: the published loop on the entry's OWN winner map and the given sized bits (per image
    bool (K, h, w)) must give the entry's areas, ids and segment map; `segment >= 0` is "the winner's bit and kept"."""
    for b, bb in enumerate(bits):
        want = panoptic(got["winner"][b], bb, overlap_threshold)
        for name in ("orig_area", "won_area", "kept_area", "segment_id"):
            assert np.array_equal(got[name][b], want[name]), (b, name, got[name][b], want[name])
        assert int(got["n_segments"][b]) == want["n_segments"], b
        assert np.array_equal(got["segment"][b], want["segment"]), b
        win = got["winner"][b]
        own = np.zeros(win.shape, bool)
        for k in range(bb.shape[0]):
            own |= (win == k) & bb[k] & (want["segment_id"][k] > 0)
        assert np.array_equal(got["segment"][b] >= 0, own), b


def sized_bits(logits: np.ndarray, sizes, level: int = 128, dev="cpu"):
    """The bits and areas cvlm_mask_pack_sized (or its host twin) writes for the same planes, sizes and level -> (per image bool
    (K, h, w), area (B, K))."""
    from camouflaged_vlm_amd import hip
    B, K, Hs, Ws = logits.shape
    per_plane = [s for s in sizes for _ in range(K)]
    entry = hip.mask_pack_sized_host if dev == "cpu" else hip.mask_pack_sized
    _, planes, area, _, status = SO.run(entry, logits.reshape(B * K, Hs, Ws), per_plane, level, dev=dev)
    assert status == 0
    bits = [np.stack([SO.unpack_rows(planes[b * K + k], sizes[b][1]) for k in range(K)]) for b in range(B)]
    return bits, area.reshape(B, K)


def compare(got: dict, logits: np.ndarray, sizes, weights=None, level: int = 128, overlap_threshold: float = 0.8, exact: bool = False,
            dev="cpu") -> int:
    """The rule of the tests for one call's outputs (State.read()).  winner: equal to the oracle's everywhere (exact), or everywhere
    but where the best and second-best fp64 score lie within MARGIN -- at most max(2, 1e-4 h w) pixels of an image, and the oracle
    itself agrees with its fp64 form outside them; the areas then differ from the oracle's by at most the pixels left out.  orig_area
    is cvlm_mask_pack_sized's area and everything behind the argmax the published loop on the entry's own winner map and those bits,
    exactly.  -> pixels left out."""
    B, K = logits.shape[:2]
    assert got["status"] == 0
    wts = None if weights is None else np.asarray(weights, np.float32).reshape(B, K)
    bits, area = sized_bits(logits, sizes, level, dev)
    assert np.array_equal(got["orig_area"], area), "orig_area is the area of the sized planes"
    check_integer_stages(got, bits, overlap_threshold)
    want = label_maps(logits, sizes, wts, level, overlap_threshold)
    total = 0
    for b, (h, w) in enumerate(sizes):
        wb = None if wts is None else wts[b]
        assert exact or wb is None or np.nanmax(np.abs(wb)) <= 1.0, "MARGIN was measured at weights up to 1"
        near = np.zeros((h, w), bool) if exact else near_ties(logits[b], h, w, wb)
        left = int(near.sum())
        diff = got["winner"][b] != want[b]["winner"]
        print(f"image {b} {(h, w)} K {K}: left out {left} of {h * w}, differing {int(diff.sum())}, segments {int(got['n_segments'][b])}")
        assert left <= max(2, 1e-4 * h * w), left
        if not exact:
            s = scores_f64(logits[b], h, w, wb)
            first = np.where(np.isnan(s).all(axis=0), -1, np.argmax(np.where(np.isnan(s), -np.inf, s), axis=0))
            assert np.array_equal(first[~near], want[b]["winner"][~near]), "the float32 oracle against its fp64 restatement"
        assert not diff[~near].any(), int(diff[~near].sum())
        assert np.abs(got["won_area"][b].astype(np.int64) - want[b]["won_area"]).max() <= left, b      # kept_area hangs on the bits too:
        #                                                           it is held exactly above, against the entry's own sized bits
        if left == 0 and exact:
            for name in ("segment", "segment_id", "orig_area", "kept_area"):
                assert np.array_equal(got[name][b], want[b][name]), (b, name)
            assert int(got["n_segments"][b]) == want[b]["n_segments"]
        total += left
    return total


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
DYADIC = (1.0, 0.5, 2.0, 0.25, 1.5, 0.75, 4.0, 0.125)
RAGGED = SO.RAGGED
SMOOTH = [((64, 64), (97, 131)), ((96, 128), (50, 201)), ((32, 64), (70, 33))]
SMOOTH_K = 5


def blocky(B: int, K: int, Hs: int, Ws: int, seed: int) -> np.ndarray:
    return np.stack([np.stack([SO.blocky(Hs, Ws, seed + 31 * b + k, block=3 + (k % 4)) for k in range(K)]) for b in range(B)])


def dyadic(B: int, K: int) -> np.ndarray:
    return np.asarray([[DYADIC[(3 * b + k) % len(DYADIC)] for k in range(K)] for b in range(B)], np.float32)


def smooth_cases():
    """-> list of (logits f32 (1, K, Hs, Ws), (h, w), weights f32 (1, K)): smooth random fields, no two planes equal, distinct weights."""
    out = []
    for i, (src, dst) in enumerate(SMOOTH):
        rng = np.random.default_rng(40 + i)
        yy, xx = np.mgrid[0:src[0], 0:src[1]]
        planes = [(5 * np.sin(yy / (9.0 + 3 * k) + k) * np.cos(xx / (13.0 + 2 * k) - k) + rng.normal(0, 1.5, src)).astype(np.float32)
                  for k in range(SMOOTH_K)]
        wts = np.asarray([[1.0, 0.93, 0.81, 0.77, 0.64]], np.float32)
        out.append((np.stack(planes)[None], dst, wts))
    return out
