"""Oracle of panoptic quality: the definition -- panopticapi.evaluation.pq_compute restated -- in plain numpy and Python
loops, the seeded generator of piecewise-constant maps, and the runner that calls the cvlm_pan_* entries (device or host) into
sentinel-filled outputs with guard bands.  Every comparison against it is exact: integers to the count, IoU and their sums as f64 bit
patterns, the oracle dividing and adding in the order the definition states."""
import numpy as np
import torch

import sized_oracle as SO

GUARD = 16
FILL_I32 = -0x5A5A5A5B
FILL_I64 = -0x5A5A5A5A5A5A5A5B
FILL_F64 = -7.25
RAGGED = SO.RAGGED


# ---- the definition ----------------------------------------------------------------------------------------------------------------------
def rgb2id(rgb: np.ndarray) -> np.ndarray:
    rgb = rgb.astype(np.int64)
    return rgb[..., 0] + 256 * rgb[..., 1] + 65536 * rgb[..., 2]


def remap(ids: np.ndarray, segments) -> tuple:
    """ids of one image, its (id, category, iscrowd) list -> (dense map int32, unknown pixels): slot i + 1 is the i-th segment."""
    slot = {int(s[0]): i + 1 for i, s in enumerate(segments)}
    flat = ids.reshape(-1)
    out = np.zeros(flat.shape, np.int32)
    unknown = 0
    for i, v in enumerate(flat.tolist()):
        if v == 0:
            continue
        if v in slot:
            out[i] = slot[v]
        else:
            unknown += 1
    return out.reshape(ids.shape), unknown


def pair_counts(gt: np.ndarray, pred: np.ndarray, G: int, S: int) -> tuple:
    """-> (inter int32 (G, S), "a pixel's index was out of range")."""
    g, s = gt.reshape(-1).astype(np.int64), pred.reshape(-1).astype(np.int64)
    ok = (g >= 0) & (g < G) & (s >= 0) & (s < S)
    return np.bincount(g[ok] * S + s[ok], minlength=G * S).astype(np.int32).reshape(G, S), bool((~ok).any())


def pair_counts_unique(gt: np.ndarray, pred: np.ndarray, G: int, S: int) -> np.ndarray:
    """The published route: np.unique over gt * 2^24 + pred (what a host evaluation runs per image)."""
    labels, cnt = np.unique(gt.reshape(-1).astype(np.uint64) * (1 << 24) + pred.reshape(-1).astype(np.uint64), return_counts=True)
    inter = np.zeros((G, S), np.int32)
    inter[(labels >> 24).astype(np.int64), (labels & ((1 << 24) - 1)).astype(np.int64)] = cnt
    return inter


def match(inter: np.ndarray, pred_cat, gt_cat, gt_crowd, C: int) -> dict:
    """Steps 2 to 4 for one image."""
    G, S = inter.shape
    cat = lambda v: int(v) if 0 <= int(v) < C else -1
    pred_area, gt_area = inter.sum(0).astype(np.int32), inter.sum(1).astype(np.int32)
    pred_match, gt_match, pred_iou = np.zeros(S, np.int32), np.zeros(G, np.int32), np.zeros(S, np.float64)
    for g in range(1, G):
        if cat(gt_cat[g]) < 0 or gt_crowd[g]:
            continue
        for s in range(1, S):
            if cat(pred_cat[s]) != cat(gt_cat[g]) or inter[g, s] <= 0:
                continue
            union = int(pred_area[s]) + int(gt_area[g]) - int(inter[g, s]) - int(inter[0, s])
            iou = np.float64(int(inter[g, s])) / np.float64(union)
            if iou > 0.5:
                assert gt_match[g] == 0 and pred_match[s] == 0, "IoU > 0.5 is unique"
                gt_match[g], pred_match[s], pred_iou[s] = s, g, iou
    crowd_of = {}
    for g in range(1, G):
        if cat(gt_cat[g]) < 0 or gt_match[g] != 0:
            continue
        if gt_crowd[g]:
            crowd_of[cat(gt_cat[g])] = g                             # the published dict overwrite: the last one wins
            gt_match[g] = -2
        else:
            gt_match[g] = -1
    for s in range(1, S):
        if cat(pred_cat[s]) < 0 or pred_area[s] <= 0 or pred_match[s] != 0:
            continue
        v = int(inter[0, s])
        if cat(pred_cat[s]) in crowd_of:
            v += int(inter[crowd_of[cat(pred_cat[s])], s])
        pred_match[s] = -2 if np.float64(v) / np.float64(int(pred_area[s])) > 0.5 else -1
    return dict(pred_match=pred_match, pred_iou=pred_iou, gt_match=gt_match, pred_area=pred_area, gt_area=gt_area)


def new_totals(C: int) -> dict:
    return dict(counts=np.zeros((3, C), np.int64), iou_sum=np.zeros(C, np.float64))


def accumulate(totals: dict, matches: list, pred_cat, gt_cat, C: int) -> dict:
    """Images in increasing b, within an image in increasing g: the order the f64 sums are formed in."""
    for b, m in enumerate(matches):
        for g in range(1, len(gt_cat[b])):
            c = int(gt_cat[b][g])
            if not 0 <= c < C:
                continue
            if m["gt_match"][g] > 0:
                totals["counts"][0, c] += 1
                totals["iou_sum"][c] = totals["iou_sum"][c] + m["pred_iou"][m["gt_match"][g]]
            elif m["gt_match"][g] == -1:
                totals["counts"][2, c] += 1
        for s in range(1, len(pred_cat[b])):
            c = int(pred_cat[b][s])
            if 0 <= c < C and m["pred_match"][s] == -1:
                totals["counts"][1, c] += 1
    return totals


def pq_compute(pred: list, pred_cat, gt: list, gt_cat, gt_crowd, C: int, totals: dict = None) -> dict:
    """Per-image maps (lists of 2-d arrays) and (B, slots) tables -> totals and the per-image results, as the entries give them."""
    pred_cat, gt_cat, gt_crowd = np.asarray(pred_cat), np.asarray(gt_cat), np.asarray(gt_crowd)
    G, S = gt_cat.shape[1], pred_cat.shape[1]
    inter, status, matches = [], 0, []
    for b in range(len(pred)):
        i, bad = pair_counts(gt[b], pred[b], G, S)
        status |= 2 * bad
        inter.append(i)
        matches.append(match(i, pred_cat[b], gt_cat[b], gt_crowd[b], C))
    totals = accumulate(new_totals(C) if totals is None else totals, matches, pred_cat, gt_cat, C)
    out = {k: np.stack([m[k] for m in matches]) for k in matches[0]}
    return dict(out, inter=np.stack(inter), status=status, counts=totals["counts"], iou_sum=totals["iou_sum"], totals=totals)


def pq_average(counts, iou_sum, isthing=None) -> dict:
    """PQStat.pq_average with Python floats, class by class."""
    groups = {"All": None} if isthing is None else {"All": None, "Things": True, "Stuff": False}
    out = {}
    for name, want in groups.items():
        pq = sq = rq = 0.0
        n = 0
        for c in range(counts.shape[1]):
            if want is not None and bool(isthing[c]) != want:
                continue
            tp, fp, fn = (int(v) for v in counts[:, c])
            if tp + fp + fn == 0:
                continue
            n += 1
            pq += float(iou_sum[c]) / (tp + 0.5 * fp + 0.5 * fn)
            sq += float(iou_sum[c]) / tp if tp != 0 else 0.0
            rq += tp / (tp + 0.5 * fp + 0.5 * fn)
        out[name] = dict(pq=pq / n, sq=sq / n, rq=rq / n, n=n) if n else dict(pq=float("nan"), sq=float("nan"), rq=float("nan"), n=0)
    return out


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- generator ------------------------------------------------------------------------------------------------------------------------------
def piecewise(h: int, w: int, n: int, seed: int, block=(5, 19)) -> np.ndarray:
    """A random piecewise-constant (h, w) int32 map over [0, n): blocks of `block` pixels, each with one label, then a few single pixels
    relabelled so that segment borders are ragged."""
    rng = np.random.default_rng(seed)
    bh, bw = block
    coarse = rng.integers(0, n, ((h + bh - 1) // bh, (w + bw - 1) // bw))
    m = np.kron(coarse, np.ones((bh, bw), np.int64))[:h, :w].astype(np.int32)
    flips = rng.random((h, w)) < 0.02
    m[flips] = rng.integers(0, n, int(flips.sum()))
    return m


def maps(sizes, G: int, S: int, seed: int) -> tuple:
    """-> (pred list, gt list): per image a predicted map over [0, S) and a ground truth that agrees with it in places (the pred
    relabelled modulo G) and differs in others, so that every kind of result occurs."""
    pred, gt = [], []
    for b, (h, w) in enumerate(sizes):
        p = piecewise(h, w, S, seed + 7 * b)
        g = np.where(piecewise(h, w, 2, seed + 7 * b + 3, (7, 23)) > 0, p % G, piecewise(h, w, G, seed + 7 * b + 5, (3, 41))).astype(np.int32)
        pred.append(p)
        gt.append(g)
    return pred, gt


def tables(B: int, G: int, S: int, C: int, seed: int) -> tuple:
    """-> (pred_cat (B, S), gt_cat (B, G), gt_crowd (B, G)): slot i's category is mostly i mod C on both sides (so pairs of equal
    category exist), a few slots unused, a few crowd."""
    rng = np.random.default_rng(seed)
    pred_cat = np.tile(np.arange(S) % C, (B, 1)).astype(np.int32)
    gt_cat = np.tile(np.arange(G) % C, (B, 1)).astype(np.int32)
    pred_cat[rng.random((B, S)) < 0.1] = -1
    gt_cat[rng.random((B, G)) < 0.1] = -1
    other = rng.random((B, G)) < 0.15
    gt_cat[other] = rng.integers(0, C, int(other.sum()))
    gt_crowd = (rng.random((B, G)) < 0.15).astype(np.uint8)
    pred_cat[:, 0] = -1
    gt_cat[:, 0] = -1
    gt_crowd[:, 0] = 0
    return pred_cat, gt_cat, gt_crowd


def shifted_gt(pred: list, pred_cat: np.ndarray, C: int, seed: int, shift=(2, 3)) -> tuple:
    """Ground truth synthesised from a prediction's own maps: every image's map shifted by `shift` pixels and its slots relabelled by a
    permutation (slot 0 stays void), the categories following their slots -- so most pairs match with IoU < 1 --, then one slot per
    image given another category and one turned into crowd -> (gt list, gt_cat (B, S), gt_crowd (B, S))."""
    rng = np.random.default_rng(seed)
    B, S = pred_cat.shape
    gt, gt_cat, gt_crowd = [], np.full((B, S), -1, np.int32), np.zeros((B, S), np.uint8)
    for b, p in enumerate(pred):
        perm = np.concatenate([[0], 1 + rng.permutation(S - 1)]).astype(np.int32)
        gt.append(perm[np.roll(p, shift, (0, 1))])
        gt_cat[b, perm] = pred_cat[b]
        used = [s for s in range(1, S) if gt_cat[b, s] >= 0]
        if len(used) >= 2:
            gt_cat[b, used[0]] = (gt_cat[b, used[0]] + 1) % C
            gt_crowd[b, used[1]] = 1
    return gt, gt_cat, gt_crowd


def shifted(sizes, n: int, C: int, seed: int) -> tuple:
    """-> (pred, gt, pred_cat, gt_cat, gt_crowd): random predictions of about n segments per image and `shifted_gt` of them."""
    rng = np.random.default_rng(seed)
    pred = [piecewise(h, w, n + 1, seed + b, (max(2, h // 5), max(2, w // 5))) for b, (h, w) in enumerate(sizes)]
    pred_cat = rng.integers(0, C, (len(sizes), n + 1)).astype(np.int32)
    pred_cat[:, 0] = -1
    gt, gt_cat, gt_crowd = shifted_gt(pred, pred_cat, C, seed + 99)
    return pred, gt, pred_cat, gt_cat, gt_crowd


# ---- runner ---------------------------------------------------------------------------------------------------------------------------------
def label_tables(sizes):
    dims = np.asarray(sizes, dtype=np.int32).reshape(-1, 2)
    pix = dims[:, 0].astype(np.int64) * dims[:, 1].astype(np.int64)
    off = np.zeros(len(sizes) + 1, np.int64)
    off[1:] = np.cumsum(pix)
    return dims, off, int(pix.max())


class Guarded:
    """A sentinel-filled tensor of `shape` that is a view GUARD elements inside a larger one."""

    def __init__(self, shape, dtype, dev):
        self.fill = {torch.int32: FILL_I32, torch.int64: FILL_I64, torch.float64: FILL_F64}[dtype]
        n = int(np.prod(shape))
        self.raw = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device=dev)
        self.t = self.raw[GUARD:GUARD + n].view(*shape)

    def read(self) -> np.ndarray:
        raw = self.raw.cpu().numpy().copy()
        assert (raw[:GUARD] == self.fill).all() and (raw[-GUARD:] == self.fill).all(), "a guard entry was overwritten"
        return raw[GUARD:-GUARD].reshape(tuple(self.t.shape))


def flat(images: list) -> np.ndarray:
    return np.concatenate([np.ascontiguousarray(m).reshape(-1) for m in images]).astype(np.int32)


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Run:
    """The four entries on `dev` ("cpu": the host entries) for images of `sizes`, every output guarded.  totals and status persist over
    calls of `score`, the per-image outputs are the last call's."""

    def __init__(self, sizes, G: int, S: int, C: int, dev="cpu", n_pix=None):
        from camouflaged_vlm_amd import hip
        self.hip, self.dev, self.host, self.sizes, self.B, self.G, self.S, self.C = hip, dev, dev == "cpu", list(sizes), len(sizes), G, S, C
        dims, self.host_off, self.max_pixels = label_tables(sizes)
        self.n = int(self.host_off[-1]) if n_pix is None else n_pix
        self.dims, self.off = up(dims, dev), up(self.host_off, dev)
        B = self.B
        i32, f64, i64 = torch.int32, torch.float64, torch.int64
        self.o = dict(inter=Guarded((B, G, S), i32, dev), status=Guarded((1,), i32, dev), pred_match=Guarded((B, S), i32, dev),
                      pred_iou=Guarded((B, S), f64, dev), gt_match=Guarded((B, G), i32, dev), pred_area=Guarded((B, S), i32, dev),
                      gt_area=Guarded((B, G), i32, dev), counts=Guarded((3, C), i64, dev), iou_sum=Guarded((C,), f64, dev))
        self.o["status"].t.zero_()

    def t(self, name):
        return self.o[name].t

    def pair_hist(self, pred, gt, zero_first=True, dims=None, off=None):
        p = pred if isinstance(pred, torch.Tensor) else up(flat(pred) if isinstance(pred, list) else pred, self.dev)
        g = gt if isinstance(gt, torch.Tensor) else up(flat(gt) if isinstance(gt, list) else gt, self.dev)
        self.hip.pan_pair_hist(p, g, self.B, self.G, self.S, self.dims if dims is None else dims, self.off if off is None else off,
                               self.max_pixels, zero_first, self.t("inter"), self.t("status"), host=self.host)

    def match(self, pred_cat, gt_cat, gt_crowd):
        self.cats = [up(np.asarray(a, dt), self.dev) for a, dt in ((pred_cat, np.int32), (gt_cat, np.int32), (gt_crowd, np.uint8))]
        self.hip.pan_match(self.t("inter"), *self.cats, self.C, self.t("pred_match"), self.t("pred_iou"), self.t("gt_match"),
                           self.t("pred_area"), self.t("gt_area"), host=self.host)

    def accumulate(self, zero_first: bool):
        self.hip.pan_accumulate(self.cats[0], self.cats[1], self.t("pred_match"), self.t("pred_iou"), self.t("gt_match"), self.C, zero_first,
                                self.t("counts"), self.t("iou_sum"), host=self.host)

    def score(self, pred, pred_cat, gt, gt_cat, gt_crowd, first: bool = True) -> dict:
        self.pair_hist(pred, gt)
        self.match(pred_cat, gt_cat, gt_crowd)
        self.accumulate(first)
        return self.read()

    def read(self) -> dict:
        if not self.host:
            torch.cuda.synchronize()
        out = {k: v.read() for k, v in self.o.items()}
        out["status"] = int(out["status"][0])
        return out


def compare(got: dict, want: dict, names=("inter", "pred_area", "gt_area", "pred_match", "gt_match", "counts", "status")) -> None:
    for n in names:
        assert np.array_equal(got[n], want[n]), n
    for n in ("pred_iou", "iou_sum"):
        assert same_bits(got[n], want[n]), n


def run_remap(raw: np.ndarray, sizes, segments, dev="cpu", rgb=False, dims=None, off=None, tab_off=None):
    """cvlm_pan_remap (or the host entry) on raw ids int32 (n_pix,) or RGB uint8 (n_pix, 3) -> (out, unknown, status), guards checked."""
    from camouflaged_vlm_amd import hip
    from camouflaged_vlm_amd.engine import pq_segments_request
    B = len(sizes)
    keys, vals, offsets, _, _ = pq_segments_request(segments, B)
    d, o, most = label_tables(sizes)
    n = int(o[-1])
    out, unknown, status = Guarded((n,), torch.int32, dev), Guarded((B,), torch.int32, dev), Guarded((1,), torch.int32, dev)
    status.t.zero_()
    hip.pan_remap(up(raw, dev), B, up(d if dims is None else dims, dev), up(o if off is None else off, dev), most, up(keys, dev), up(vals, dev),
                  up(offsets if tab_off is None else tab_off, dev), out.t, unknown.t, status.t, host=dev == "cpu")
    if dev != "cpu":
        torch.cuda.synchronize()
    return out.read(), unknown.read(), int(status.read()[0])


# ---- known answers: hand-written maps of a few pixels ---------------------------------------------------------------------------------------
# name -> (gt pixels, gt_cat, gt_crowd, pred pixels, pred_cat, C, tp, fp, fn, iou_sum) of ONE image of one row
KNOWN = {
    # three segments of three classes scored against themselves
    "identity": ([1, 1, 2, 2, 3, 3], [-1, 0, 1, 2], [0, 0, 0, 0], [1, 1, 2, 2, 3, 3], [-1, 0, 1, 2], 3, [1, 1, 1], [0, 0, 0], [0, 0, 0], [1.0, 1.0, 1.0]),
    # gt {a, b, c}, pred {b, c, d}: inter 2, union 4, IoU exactly one half: no match (d lies on another gt segment, a on pred void)
    "half": ([1, 1, 1, 2], [-1, 0, 1], [0, 0, 0], [0, 1, 1, 1], [-1, 0], 2, [0, 0], [1, 0], [1, 1], [0.0, 0.0]),
    # gt {a, b, c, d}, pred {b, c, d, e}: inter 3, union 5, IoU 0.6
    "three_fifths": ([1, 1, 1, 1, 2], [-1, 0, 1], [0, 0, 0], [0, 1, 1, 1, 1], [-1, 0], 2, [1, 0], [0, 0], [0, 1], [3 / 5, 0.0]),
    # pred has 6 pixels, 4 on a gt segment of 4 and 2 on void: union 6 + 4 - 4 - 2 = 4, IoU 1.0
    "void_subtraction": ([1, 1, 1, 1, 0, 0], [-1, 0], [0, 0], [1] * 6, [-1, 0], 1, [1], [0], [0], [1.0]),
    "other_class": ([1, 1], [-1, 0], [0, 0], [1, 1], [-1, 1], 2, [0, 0], [0, 1], [1, 0], [0.0, 0.0]),
    # a crowd segment under 3 of 4 pixels of an unmatched pred of its class: pred ignored, crowd never FN
    "crowd_ignores": ([1, 1, 1, 2], [-1, 0, 1], [0, 1, 0], [1, 1, 1, 1], [-1, 0], 2, [0, 0], [0, 0], [0, 1], [0.0, 0.0]),
    # under exactly half: FP
    "crowd_half": ([1, 1, 2, 2], [-1, 0, 1], [0, 1, 0], [1, 1, 1, 1], [-1, 0], 2, [0, 0], [1, 0], [0, 1], [0.0, 0.0]),
    # two crowd segments of one class: only the later slot (1 of 5 pixels) counts; the earlier one (3 of 5) would have ignored it
    "crowd_last_wins": ([1, 1, 1, 2, 3], [-1, 0, 0, 1], [0, 1, 1, 0], [1] * 5, [-1, 0], 2, [0, 0], [1, 0], [0, 1], [0.0, 0.0]),
    # a crowd with IoU 1 against a pred: no TP; the pred is ignored
    "crowd_no_tp": ([1, 1], [-1, 0], [0, 1], [1, 1], [-1, 0], 1, [0], [0], [0], [0.0]),
    "gt_slot_without_pixel": ([1, 1], [-1, 0, 1], [0, 0, 0], [1, 1], [-1, 0], 2, [1, 0], [0, 0], [0, 1], [1.0, 0.0]),
    "pred_slot_without_pixel": ([1, 1], [-1, 0], [0, 0], [1, 1], [-1, 0, 1], 2, [1, 0], [0, 0], [0, 0], [1.0, 0.0]),
    "unused_slots": ([1, 1, 2, 2], [-1, 0, -1], [0, 0, 0], [1, 1, 2, 2], [-1, 0, -1], 1, [1], [0], [0], [1.0]),
}


def case_known(dev: str) -> None:
    for name, (gt, gt_cat, crowd, pred, pred_cat, C, tp, fp, fn, iou_sum) in KNOWN.items():
        g, p = [np.asarray([gt], np.int32)], [np.asarray([pred], np.int32)]
        want = pq_compute(p, [pred_cat], g, [gt_cat], [crowd], C)
        assert want["counts"].tolist() == [tp, fp, fn] and same_bits(want["iou_sum"], np.asarray(iou_sum, np.float64)), name
        got = Run([(1, len(gt))], len(gt_cat), len(pred_cat), C, dev).score(p, [pred_cat], g, [gt_cat], [crowd])
        compare(got, want)
    ident = pq_average(np.asarray([[1, 1, 1], [0, 0, 0], [0, 0, 0]]), np.ones(3))
    assert ident["All"] == dict(pq=1.0, sq=1.0, rq=1.0, n=3)


# ---- the shapes of the pair histogram ---------------------------------------------------------------------------------------------------------
WIDTHS, HEIGHTS = (1, 63, 64, 65, 257), (1, 2, 33)


def factor(n: int) -> tuple:
    """n = G * S with G <= S as close to each other as n allows."""
    g = int(np.sqrt(n))
    while n % g:
        g -= 1
    return g, n // g


def slot_shapes() -> list:
    from camouflaged_vlm_amd import hip
    L = hip.pan_lds_cells()
    return [(1, 1), (2, 2), (21, 62), factor(L), factor(L + 1)]          # the last two: the LDS path's last table, the global path's first


def scored(sizes, G: int, S: int, C: int, seed: int, dev: str, pred=None, gt=None) -> tuple:
    """One full sequence on random maps and tables, held against the oracle -> (Run, got, inputs)."""
    if pred is None:
        pred, gt = maps(sizes, G, S, seed)
    pred_cat, gt_cat, gt_crowd = tables(len(sizes), G, S, C, seed + 1)
    run = Run(sizes, G, S, C, dev)
    got = run.score(pred, pred_cat, gt, gt_cat, gt_crowd)
    compare(got, pq_compute(pred, pred_cat, gt, gt_cat, gt_crowd, C))
    for b, (h, w) in enumerate(sizes):                               # every pixel once; row and column sums are the maps' bincounts
        assert int(got["inter"][b].sum()) == h * w
        assert np.array_equal(got["inter"][b].sum(1), np.bincount(gt[b].reshape(-1), minlength=G))
        assert np.array_equal(got["inter"][b].sum(0), np.bincount(pred[b].reshape(-1), minlength=S))
    return run, got, (pred, pred_cat, gt, gt_cat, gt_crowd)


def case_widths_and_heights(dev: str) -> None:
    for w in WIDTHS:
        for h in HEIGHTS:
            scored([(h, w)], 21, 62, 7, 100 * h + w, dev)


def case_slot_shape(dev: str, G: int, S: int) -> None:
    scored(RAGGED, G, S, 5, G + S, dev)
    _, got, _ = scored([(33, 257)], G, S, 5, G * S, dev)
    assert G * S == 1 or (got["inter"][0] > 0).sum() > 1


def case_uniform_and_checkered(dev: str) -> None:
    """One cell throughout: all 64 lanes agree in every unit.  Then a map in which no two lanes of a wave agree."""
    h, w = 5, 130
    pred, gt = [np.full((h, w), 3, np.int32)], [np.full((h, w), 2, np.int32)]
    _, got, _ = scored([(h, w)], 4, 5, 3, 1, dev, pred, gt)
    assert got["inter"][0, 2, 3] == h * w and (got["inter"] > 0).sum() == 1
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    pred, gt = [((x + y) % 64).astype(np.int32)], [((x + 2 * y) % 3).astype(np.int32)]
    scored([(h, w)], 3, 64, 3, 2, dev, pred, gt)


def case_accumulating_calls(dev: str) -> None:
    """Two pair-histogram calls without zero_first equal one call over both sets of maps; zero_first clears a used table; the whole
    sequence twice into used outputs gives the first result; a map whose base is 4 bytes off a 16-byte boundary."""
    G, S, C = 21, 62, 7
    run, first, (pred, pred_cat, gt, gt_cat, gt_crowd) = scored(RAGGED, G, S, C, 11, dev)
    pred2, gt2 = maps(RAGGED, G, S, 12)
    run.pair_hist(pred2, gt2, zero_first=False)
    both = run.read()["inter"]
    want2 = pq_compute(pred2, pred_cat, gt2, gt_cat, gt_crowd, C)
    assert np.array_equal(both, first["inter"] + want2["inter"])
    run.pair_hist(pred2, gt2, zero_first=True)
    assert np.array_equal(run.read()["inter"], want2["inter"])
    again = run.score(pred, pred_cat, gt, gt_cat, gt_crowd)
    compare(again, first)
    n = int(run.host_off[-1])
    room = torch.zeros(n + 8, dtype=torch.int32, device=dev)
    base = (-room.data_ptr() // 4) % 4
    shifted = room[base + 1:base + 1 + n]
    assert shifted.data_ptr() % 16 == 4
    shifted.copy_(up(flat(pred), dev))
    run.pair_hist(shifted, gt)
    assert np.array_equal(run.read()["inter"], first["inter"])


def case_out_of_range_index(dev: str) -> None:
    G, S, C = 5, 6, 3
    pred, gt = maps(RAGGED, G, S, 21)
    for which, value in ((pred, S), (pred, -1), (gt, G), (gt, 2 ** 31 - 1)):
        p, g = [m.copy() for m in pred], [m.copy() for m in gt]
        (p if which is pred else g)[5][40, 100] = value
        pred_cat, gt_cat, gt_crowd = tables(7, G, S, C, 3)
        run = Run(RAGGED, G, S, C, dev)
        got = run.score(p, pred_cat, g, gt_cat, gt_crowd)
        want = pq_compute(p, pred_cat, g, gt_cat, gt_crowd, C)
        assert got["status"] == 2 and want["status"] == 2 and int(got["inter"][5].sum()) == 97 * 131 - 1
        compare(got, want)


def case_refused_image(dev: str) -> None:
    """A bad table entry: status 1, the image's table stays zero, its neighbours' are whole."""
    G, S, C = 5, 6, 3
    pred, gt = maps(RAGGED, G, S, 31)
    good = pq_compute(pred, *tables(7, G, S, C, 3)[:1], gt, *tables(7, G, S, C, 3)[1:], C)["inter"]
    dims, off, _ = label_tables(RAGGED)
    cases = []
    bad = off.copy(); bad[3:] += 1
    cases.append(dict(off=bad, skipped=(2,), n_pix=int(off[-1]) + 1))
    bad = off.copy(); bad[2] -= 1
    cases.append(dict(off=bad, skipped=(1, 2)))
    for hw in ((0, 65), (5, 0), (-5, 65), (5, 16385), (2 ** 31 - 1, 2 ** 31 - 1)):
        d = dims.copy(); d[2] = hw
        cases.append(dict(dims=d, skipped=(2,)))
    cases.append(dict(n_pix=int(off[-1]) - 1, skipped=(6,)))
    bad = off.copy(); bad[0] = -1
    cases.append(dict(off=bad, skipped=(0,)))
    for case in cases:
        n = case.get("n_pix", int(off[-1]))
        run = Run(RAGGED, G, S, C, dev, n_pix=n)
        fp, fg = np.zeros(n, np.int32), np.zeros(n, np.int32)
        m = min(n, int(off[-1]))
        fp[:m], fg[:m] = flat(pred)[:m], flat(gt)[:m]
        run.pair_hist(fp, fg, dims=up(case["dims"], dev) if "dims" in case else None, off=up(case["off"], dev) if "off" in case else None)
        got = run.read()
        assert got["status"] == 1, case
        for b in range(7):
            if b in case["skipped"]:
                assert not got["inter"][b].any(), (case, b)
            elif "off" not in case or all(case["off"][b:b + 2] == off[b:b + 2]):
                assert np.array_equal(got["inter"][b], good[b]), (case, b)
            else:                                                    # a whole image read one pixel further on
                assert int(got["inter"][b].sum()) == RAGGED[b][0] * RAGGED[b][1], (case, b)


def case_accumulate(dev: str, B: int, C: int) -> None:
    """Totals over two batches equal the oracle's over both, iou_sum to the bit."""
    sizes = [RAGGED[(b % 6) + 1] for b in range(B)]
    G, S = 9, 11
    run = Run(sizes, G, S, C, dev)
    totals = None
    for batch in range(2):
        pred, gt = maps(sizes, G, S, 1000 * batch + C)
        pred_cat, gt_cat, gt_crowd = tables(B, G, S, C, batch + 5)
        if C > G:                                                    # spread the slots over all of the classes, the last one included
            spread = np.random.default_rng(batch).integers(0, C, (B, G)).astype(np.int32)
            spread[:, 1] = C - 1
            spread[:, 0] = -1
            gt_cat = spread
            pred_cat = np.concatenate([spread, spread[:, 1:3]], axis=1)
        got = run.score(pred, pred_cat, gt, gt_cat, gt_crowd, first=batch == 0)
        want = pq_compute(pred, pred_cat, gt, gt_cat, gt_crowd, C, totals)
        totals = want["totals"]
        compare(got, want)
    assert got["counts"].sum() > 0
