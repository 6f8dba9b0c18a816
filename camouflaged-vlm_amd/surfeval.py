"""Surface-distance metrics from directed surface totals: pure numpy on the host, float64.

`surface_metrics` takes what `SurfaceTotals.to_host()` returns -- for N pairs the totals `ab` of the prediction's surface pixels against
the truth's distance map and `ba` of the reverse, each with n, far, within (N, T), max_d2, sum_d2, sum_d -- and returns per-pair arrays:

  hausdorff      sqrt(max(max_d2 of ab, max_d2 of ba)); 0.0 when both surfaces are empty, inf when exactly one is empty or a pixel
                 of either direction was far (the maps were cut at a reach: ask for reach=None)
  assd           (sum_d of ab + sum_d of ba) / (n of ab + n of ba): the average symmetric surface distance; the same empty cases
  nsd[k]         (within_ab[k] + within_ba[k]) / (n_ab + n_ba): the normalised surface Dice at tolerance k; 1.0 when both surfaces are
                 empty, 0.0 when one is
  precision[k]   within_ab[k] / n_ab, recall[k] = within_ba[k] / n_ba and f[k] = 2 P R / (P + R), 0.0 where P + R = 0: the boundary
                 F-measure at tolerance k.  An empty prediction against a non-empty truth has P = 1, R = 0; the reverse P = 0, R = 1;
                 both empty P = R = 1.

A tolerance r counts D2 <= r^2, which is exactly a dilation by the disc {dx^2 + dy^2 <= r^2} -- the structuring element the published
boundary F-measure dilates with.  The surface is whatever the totals were taken over: Cascade.mask_surface_distances' default is the
boundary at radius 1 of DESIGN.md §25, not the published measure's own seg2bmap.  A refused pair (n = -1) gives NaN everywhere."""
import numpy as np


def surface_metrics(totals_host: dict) -> dict:
    ab, ba = totals_host["ab"], totals_host["ba"]
    na, nb = np.asarray(ab["n"], dtype=np.float64), np.asarray(ba["n"], dtype=np.float64)
    wa, wb = np.asarray(ab["within"], dtype=np.float64), np.asarray(ba["within"], dtype=np.float64)
    refused = (na < 0) | (nb < 0)
    both = (na == 0) & (nb == 0)
    one = ((na == 0) | (nb == 0)) & ~both
    cut = (np.asarray(ab["far"]) != 0) | (np.asarray(ba["far"]) != 0)
    both_, one_ = both[:, None], one[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        hd = np.sqrt(np.maximum(ab["max_d2"], ba["max_d2"]).astype(np.float64))
        assd = (np.asarray(ab["sum_d"], dtype=np.float64) + np.asarray(ba["sum_d"], dtype=np.float64)) / (na + nb)
        nsd = (wa + wb) / (na + nb)[:, None]
        prec, rec = wa / na[:, None], wb / nb[:, None]
    hd = np.where(both, 0.0, np.where(one | cut, np.inf, hd))
    assd = np.where(both, 0.0, np.where(one | cut, np.inf, assd))
    nsd = np.where(both_, 1.0, np.where(one_, 0.0, nsd))
    prec = np.where(both_ | (na == 0)[:, None], 1.0, np.where(one_, 0.0, prec))
    rec = np.where(both_ | (nb == 0)[:, None], 1.0, np.where(one_, 0.0, rec))
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(prec + rec == 0, 0.0, 2 * prec * rec / (prec + rec))
    out = dict(hausdorff=hd, assd=assd, nsd=nsd, precision=prec, recall=rec, f=f)
    for k, v in out.items():
        out[k] = np.where(refused if v.ndim == 1 else refused[:, None], np.nan, v)
    return out


def cldice(totals_host: dict) -> dict:
    """Centre-line Dice (clDice, Shit et al., CVPR 2021) from what `ClDiceTotals.to_host()` returns -- for N pairs
    skel_a = |S_A|, skel_a_in_b = |S_A & B|, skel_b = |S_B|, skel_b_in_a = |S_B & A| with S_X the thinned X -- in float64 -> per-pair
    arrays tprec = skel_a_in_b / skel_a, tsens = skel_b_in_a / skel_b and cldice = 2 tprec tsens / (tprec + tsens).  A non-empty mask
    never has an empty skeleton, so the skeleton counts say which side is empty: both empty give cldice = tprec = tsens = 1; exactly
    one empty gives cldice = 0 (the empty side's own ratio 1, the other's 0, as the boundary F-measure has it); tprec + tsens = 0
    gives 0.  A refused pair (an intersection of -1: two sizes that differ) gives NaN everywhere."""
    sa, sb = np.asarray(totals_host["skel_a"], dtype=np.float64), np.asarray(totals_host["skel_b"], dtype=np.float64)
    ia, ib = np.asarray(totals_host["skel_a_in_b"], dtype=np.float64), np.asarray(totals_host["skel_b_in_a"], dtype=np.float64)
    refused = (ia < 0) | (ib < 0) | (sa < 0) | (sb < 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        tp = np.where(sa == 0, 1.0, np.where(sb == 0, 0.0, ia / sa))
        ts = np.where(sb == 0, 1.0, np.where(sa == 0, 0.0, ib / sb))
        cl = np.where(tp + ts == 0, 0.0, 2 * tp * ts / (tp + ts))
    cl = np.where((sa == 0) & (sb == 0), 1.0, np.where((sa == 0) | (sb == 0), 0.0, cl))
    return {k: np.where(refused, np.nan, v) for k, v in dict(tprec=tp, tsens=ts, cldice=cl).items()}
