"""The published COCO evaluation, loop for loop: `evaluate_img` is COCOeval.evaluateImg, `accumulate` and `summarize`
are COCOeval.accumulate / summarize, `ious_of` is rleIou's quotient from integers.  Two departures, both stated in §22: "matched" is an
index >= 0 (the published `gtm > 0` misreads id 0), and ids are the positions in the group's own tables.  `argmax_form` is the
sort-free restatement the kernel runs; tests/test_match_cpu.py holds it against the loop.  Pure numpy; `run_entry` calls
cvlm_coco_match or its host entry on a list of groups."""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNGS = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
MAX_DETS = (1, 10, 100)


def ious_of(inter, det_area, gt_area, iscrowd):
    """(D, G) float64: inter / (area_d + area_g - inter), inter / area_d against a crowd annotation, 0 for inter = 0, -1 for inter < 0."""
    inter = np.asarray(inter, dtype=np.int64).reshape(len(det_area), len(gt_area))
    out = np.zeros(inter.shape, dtype=np.float64)
    for d in range(inter.shape[0]):
        for g in range(inter.shape[1]):
            i = int(inter[d, g])
            if i < 0:
                out[d, g] = -1.0
            elif i > 0:
                u = int(det_area[d]) if iscrowd[g] else int(det_area[d]) + int(gt_area[g]) - i
                out[d, g] = float(i) / float(u)
    return out


def evaluate_img(ious, det_area, scores, range_area, iscrowd, a_rng, max_det, iou_thrs=IOU_THRS):
    """COCOeval.evaluateImg for one group and one area range -> dict(order, dtm [T, D'], dt_ig [T, D'], gtm [T, G] and gt_ig [G] in the
    caller's annotation order, scores [D'] in rank order); order[r] = the caller's row of the detection of rank r, D' = min(D, max_det);
    dtm / gtm hold caller's rows or -1."""
    G, D0 = len(range_area), len(scores)
    gt_ig_caller = np.array([1 if (iscrowd[g] or range_area[g] < a_rng[0] or range_area[g] > a_rng[1]) else 0 for g in range(G)], dtype=np.int64)
    gtind = np.argsort(gt_ig_caller, kind="mergesort")
    dtind = np.argsort(-np.asarray(scores, dtype=np.float32), kind="mergesort")[:max_det]
    io = ious[dtind][:, gtind] if G and D0 else np.zeros((0, 0))
    crowd = [int(bool(iscrowd[g])) for g in gtind]
    gt_ig = gt_ig_caller[gtind]
    T, D = len(iou_thrs), len(dtind)
    gtm = -np.ones((T, G), dtype=np.int64)
    dtm = -np.ones((T, D), dtype=np.int64)
    dt_ig = np.zeros((T, D), dtype=bool)
    if io.size:
        for tind, t in enumerate(iou_thrs):
            for dind in range(D):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind in range(G):
                    if gtm[tind, gind] >= 0 and not crowd[gind]:
                        continue
                    if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                        break
                    if io[dind, gind] < iou:
                        continue
                    iou = io[dind, gind]
                    m = gind
                if m == -1:
                    continue
                dt_ig[tind, dind] = gt_ig[m]
                dtm[tind, dind] = gtind[m]
                gtm[tind, m] = dtind[dind]
    a = np.array([det_area[d] < a_rng[0] or det_area[d] > a_rng[1] for d in dtind], dtype=bool).reshape((1, D))
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm < 0, np.repeat(a, T, 0)))
    gtm_caller = -np.ones((T, G), dtype=np.int64)
    gtm_caller[:, gtind] = gtm
    return dict(order=dtind.astype(np.int64), dtm=dtm, dt_ig=dt_ig, gtm=gtm_caller, gt_ig=gt_ig_caller.astype(bool),
                scores=np.asarray(scores, dtype=np.float32)[dtind])


def argmax_form(ious, det_area, scores, range_area, iscrowd, a_rng, max_det, iou_thrs=IOU_THRS):
    """The same results without a sort of the annotations: among the annotations not ignored that are unmatched or crowd the largest
    IoU >= the threshold, the largest index on ties; only if there is none, the same among the ignored ones."""
    G, D0 = len(range_area), len(scores)
    s = np.asarray(scores, dtype=np.float32)

    def before(j, i):
        nj, ni = bool(np.isnan(s[j])), bool(np.isnan(s[i]))
        if nj or ni:
            return j < i if nj == ni else ni
        return bool(s[j] > s[i]) or (bool(s[j] == s[i]) and j < i)

    rank = [sum(before(j, i) for j in range(D0)) for i in range(D0)]
    order = np.empty(D0, dtype=np.int64)
    order[rank] = np.arange(D0)
    order = order[:max_det]
    D, T = len(order), len(iou_thrs)
    ig = np.array([bool(iscrowd[g] or range_area[g] < a_rng[0] or range_area[g] > a_rng[1]) for g in range(G)], dtype=bool)
    gtm = -np.ones((T, G), dtype=np.int64)
    dtm = -np.ones((T, D), dtype=np.int64)
    dt_ig = np.zeros((T, D), dtype=bool)
    for ti, t in enumerate(iou_thrs):
        thr = min(t, 1 - 1e-10)
        for di, d in enumerate(order):
            m = -1
            for cls in (False, True):
                best = thr
                for g in range(G):
                    if ig[g] != cls or (gtm[ti, g] >= 0 and not iscrowd[g]):
                        continue
                    if ious[d, g] >= best:
                        best, m = ious[d, g], g
                if m >= 0:
                    break
            if m < 0:
                dt_ig[ti, di] = det_area[d] < a_rng[0] or det_area[d] > a_rng[1]
                continue
            dt_ig[ti, di], dtm[ti, di], gtm[ti, m] = ig[m], m, d
    return dict(order=order, dtm=dtm, dt_ig=dt_ig, gtm=gtm, gt_ig=ig, scores=s[order])


def evaluate_group(group, iou_thrs=IOU_THRS, area_rngs=AREA_RNGS, max_det=100, form=evaluate_img):
    """A group -- dict(inter (D, G), det_area, scores, gt_area, range_area (None: gt_area), iscrowd) -- in every area range -> list of A
    evaluate_img results."""
    ra = group["gt_area"] if group.get("range_area") is None else group["range_area"]
    ious = ious_of(group["inter"], group["det_area"], group["gt_area"], group["iscrowd"])
    return [form(ious, group["det_area"], group["scores"], ra, group["iscrowd"], rng, max_det, iou_thrs) for rng in area_rngs]


def accumulate(eval_imgs, K, A, max_dets=MAX_DETS, iou_thrs=IOU_THRS, rec_thrs=REC_THRS):
    """COCOeval.accumulate.  eval_imgs[k][a] = the list of evaluate_img results (or None) of category k and area range a over the
    images, in image order -> dict(precision [T, R, K, A, M], recall [T, K, A, M], scores [T, R, K, A, M])."""
    T, R, M = len(iou_thrs), len(rec_thrs), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k in range(K):
        for a in range(A):
            for m, max_det in enumerate(max_dets):
                E = [e for e in eval_imgs[k][a] if e is not None]
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([e["scores"][0:max_det] for e in E])
                inds = np.argsort(-dt_scores, kind="mergesort")
                dt_scores_sorted = dt_scores[inds]
                dtm = np.concatenate([e["dtm"][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dt_ig"][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gt_ig"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm >= 0, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm >= 0), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp = np.array(tp)
                    fp = np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    ss = np.zeros((R,))
                    if nd:
                        recall[t, k, a, m] = rc[-1]
                    else:
                        recall[t, k, a, m] = 0
                    pr = pr.tolist()
                    q = q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds_r = np.searchsorted(rc, rec_thrs, side="left")
                    try:
                        for ri, pi in enumerate(inds_r):
                            q[ri] = pr[pi]
                            ss[ri] = dt_scores_sorted[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
                    scores[t, :, k, a, m] = np.array(ss)
    return dict(precision=precision, recall=recall, scores=scores, iou_thrs=np.asarray(iou_thrs), max_dets=tuple(max_dets))


def summarize(acc):
    """COCOeval.summarize's twelve numbers (the default parameters' area ranges all / small / medium / large)."""
    thrs, max_dets = acc["iou_thrs"], acc["max_dets"]

    def one(ap, iou=None, a=0, m=len(max_dets) - 1):
        s = acc["precision"] if ap else acc["recall"]
        if iou is not None:
            s = s[np.where(iou == thrs)[0]]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))

    return [one(1), one(1, iou=.5), one(1, iou=.75), one(1, a=1), one(1, a=2), one(1, a=3),
            one(0, m=0), one(0, m=1), one(0, m=2), one(0, a=1), one(0, a=2), one(0, a=3)]


# ---- the C entries on lists of groups ---------------------------------------------------------------------------------------------------
def tables(groups):
    """The flat tables of cvlm_coco_match for a list of groups, as numpy arrays."""
    D = [len(g["scores"]) for g in groups]
    G = [len(g["gt_area"]) for g in groups]
    cat = lambda key, dt: np.concatenate([np.asarray(g[key], dtype=dt).reshape(-1) for g in groups] + [np.zeros(0, dtype=dt)])
    ra = np.concatenate([np.asarray(g["gt_area"] if g.get("range_area") is None else g["range_area"], dtype=np.float64).reshape(-1)
                         for g in groups] + [np.zeros(0)])
    return dict(det_offsets=np.concatenate([[0], np.cumsum(D)]).astype(np.int32), gt_offsets=np.concatenate([[0], np.cumsum(G)]).astype(np.int32),
                pair_offsets=np.concatenate([[0], np.cumsum([d * g for d, g in zip(D, G)])]).astype(np.int64), inter=cat("inter", np.int32),
                det_area=cat("det_area", np.int32), score=cat("scores", np.float32), gt_area=cat("gt_area", np.int32), gt_range_area=ra,
                gt_crowd=cat("iscrowd", np.uint8))


def run_entry(fn, tabs, iou_thrs=IOU_THRS, area_rngs=AREA_RNGS, max_det=100, dev="cpu", outs=None, guard=0):
    """One call of hip.coco_match / hip.coco_match_host on `tabs` (tables(), possibly doctored) -> dict of numpy outputs and `status`.
    outs: tensors of an earlier call to write into again.  guard: elements of sentinel before and behind every output, checked."""
    import torch
    T, A = len(iou_thrs), len(area_rngs)
    ND, NG = len(tabs["det_area"]), len(tabs["gt_area"])
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    shapes = dict(dt_order=((ND,), torch.int32), dt_match=((A, T, ND), torch.int32), dt_ignore=((A, T, ND), torch.uint8),
                  gt_match=((A, T, NG), torch.int32), gt_ignore=((A, NG), torch.uint8), status=((1,), torch.int32))
    if outs is None:
        outs = {}
        for k, (shape, dt) in shapes.items():
            n = int(np.prod(shape))
            pad = (guard + 7) // 8 * 8                                  # keeps the 4-byte alignment of what follows
            outs[k + "_buf"] = torch.full((n + 2 * pad,), 77, dtype=dt, device=dev)
            outs[k] = outs[k + "_buf"][pad:pad + n].view(shape)
    fn(dv(tabs["det_offsets"]), dv(tabs["gt_offsets"]), dv(tabs["pair_offsets"]), dv(tabs["inter"]), dv(tabs["det_area"]), dv(tabs["score"]),
       dv(tabs["gt_area"]), dv(tabs["gt_range_area"]), dv(tabs["gt_crowd"]), dv(np.asarray(iou_thrs, dtype=np.float64)),
       dv(np.asarray(area_rngs, dtype=np.float64).reshape(A, 2)), max_det, *(outs[k] for k in shapes))
    res = {k: outs[k].cpu().numpy() for k in shapes}
    for k, (shape, _) in shapes.items():
        buf, n = outs[k + "_buf"].cpu().numpy(), int(np.prod(shape))
        pad = (buf.size - n) // 2
        assert (buf[:pad] == 77).all() and (buf[pad + n:] == 77).all(), f"{k}: a guard band was written"
    res["outs"] = outs
    res["status"] = int(res["status"][0])
    return res


def check_groups(res, groups, iou_thrs=IOU_THRS, area_rngs=AREA_RNGS, max_det=100, which=None, refused=()):
    """The outputs of run_entry against evaluate_group, group by group, every byte: `refused` groups hold the fill."""
    d_off = np.concatenate([[0], np.cumsum([len(g["scores"]) for g in groups])])
    g_off = np.concatenate([[0], np.cumsum([len(g["gt_area"]) for g in groups])])
    for e, grp in enumerate(groups):
        if which is not None and e not in which:
            continue
        d0, d1, g0, g1 = d_off[e], d_off[e + 1], g_off[e], g_off[e + 1]
        if e in refused:
            assert (res["dt_order"][d0:d1] == -1).all() and (res["dt_match"][:, :, d0:d1] == -1).all()
            assert (res["dt_ignore"][:, :, d0:d1] == 1).all() and (res["gt_match"][:, :, g0:g1] == -1).all()
            assert (res["gt_ignore"][:, g0:g1] == 1).all()
            continue
        want = evaluate_group(grp, iou_thrs, area_rngs, max_det)
        full = evaluate_group(grp, iou_thrs, area_rngs[:1], 1 << 30)[0]["order"]
        assert np.array_equal(res["dt_order"][d0:d1], d0 + full), e
        for a, w in enumerate(want):
            R = len(w["order"])
            assert np.array_equal(res["dt_match"][a, :, d0:d0 + R], np.where(w["dtm"] >= 0, g0 + w["dtm"], -1)), (e, a)
            assert np.array_equal(res["dt_ignore"][a, :, d0:d0 + R], w["dt_ig"].astype(np.uint8)), (e, a)
            assert (res["dt_match"][a, :, d0 + R:d1] == -1).all() and (res["dt_ignore"][a, :, d0 + R:d1] == 1).all(), (e, a)
            assert np.array_equal(res["gt_match"][a, :, g0:g1], np.where(w["gtm"] >= 0, d0 + w["gtm"], -1)), (e, a)
            assert np.array_equal(res["gt_ignore"][a, g0:g1], w["gt_ig"].astype(np.uint8)), (e, a)
