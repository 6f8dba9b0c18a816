"""CPU: connected components of packed masks -- the scipy oracle (tests/components_oracle.py) against a plain flood
fill, cvlm_debug_mask_components_host (the kernels' per-thread functions run sequentially on the CPU) against the oracle on every
operator case and on the reference's own planes (tests/golden/demo_classes_digest.npz), the refusals of the entries (no GPU needed:
they refuse before launching) and the host check of the engine's arguments (engine.components_request)."""
import dataclasses
import os
from collections import deque

import numpy as np
import pytest
import torch

from camouflaged_vlm_amd import hip, spec
from camouflaged_vlm_amd.engine import ClassHypotheses, components_request
import compact_oracle as XO
import components_oracle as CC


def host_components(bits: np.ndarray, H: int, W: int, connectivity: int, M: int, min_area: int) -> dict:
    """cvlm_debug_mask_components_host into sentinel-filled outputs -> the oracle's dict."""
    P = bits.shape[0]
    b = torch.from_numpy(np.ascontiguousarray(bits))
    out = dict(n_comp=torch.full((P,), -7, dtype=torch.int32))
    if M:
        out["comps"] = torch.full((P, M, 6), -7, dtype=torch.int32)
    if min_area:
        out.update(n_kept=torch.full((P,), -7, dtype=torch.int32), kept_bits=torch.full_like(b, 0xa5),
                   kept_area=torch.full((P,), -7, dtype=torch.int32), kept_box=torch.full((P, 4), -7, dtype=torch.int32))
    hip.mask_components_host(b, H, W, connectivity, min_area, **out)
    return {k: v.numpy() for k, v in out.items()}


def assert_equal(got: dict, want: dict, what) -> None:
    assert set(got) <= set(want), what
    for k, v in got.items():
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), (what, k)


def flood_fill(plane: np.ndarray, connectivity: int):
    """The plainest labelling there is: raster scan, breadth-first fill -> rows (area, x0, y0, x1, y1, seed) sorted by (-area, seed)."""
    H, W = plane.shape
    seen = np.zeros_like(plane)
    steps = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 8 else [])
    rows = []
    for y in range(H):
        for x in range(W):
            if not plane[y, x] or seen[y, x]:
                continue
            seen[y, x] = True
            todo, px = deque([(y, x)]), []
            while todo:
                cy, cx = todo.popleft()
                px.append((cy, cx))
                for dy, dx in steps:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < H and 0 <= nx < W and plane[ny, nx] and not seen[ny, nx]:
                        seen[ny, nx] = True
                        todo.append((ny, nx))
            ys, xs = [p[0] for p in px], [p[1] for p in px]
            rows.append((len(px), min(xs), min(ys), max(xs), max(ys), y * W + x))
    return sorted(rows, key=lambda r: (-r[0], r[5]))


def test_oracle_equals_flood_fill():
    rng = np.random.default_rng(5)
    planes = [rng.random((8, 32)) < d for d in (0.1, 0.2, 0.3, 0.4, 0.5, 0.55, 0.6, 0.7, 0.8, 0.9)]
    planes += [np.zeros((8, 32), bool), np.ones((8, 32), bool)]
    for plane in planes:
        for conn in (4, 8):
            want = flood_fill(plane, conn)
            _, rows = CC.regions(plane, conn)
            assert rows.tolist() == [list(r) for r in want]
            got = CC.components(CC.pack(plane[None]), 8, 32, conn, M=3, min_area=2)
            assert got["n_comp"][0] == len(want) and got["n_kept"][0] == sum(r[0] >= 2 for r in want)
            assert got["comps"][0].tolist() == [list(r) for r in want[:3]] + [list(CC.FILLER)] * max(0, 3 - len(want))


def _min_areas(bits, H, W):
    return (0, 1, 3, int(XO.stats(XO.unpack(bits, H, W))[0].max()) + 1)     # the last: above any region's area


@pytest.mark.parametrize("name", sorted(CC.operator_cases()))
def test_host_entry_equals_oracle_on_operator_cases(name):
    planes = CC.operator_cases()[name]
    P, H, W = planes.shape
    bits = CC.pack(planes)
    for conn in (4, 8):
        for M in (1, 5):
            for min_area in _min_areas(bits, H, W):
                assert_equal(host_components(bits, H, W, conn, M, min_area), CC.components(bits, H, W, conn, M, min_area),
                             (name, conn, M, min_area))
    got = host_components(bits, H, W, 8, 0, 0)                                   # no table, nothing kept: the count alone
    assert list(got) == ["n_comp"] and np.array_equal(got["n_comp"], CC.components(bits, H, W, 8, 1, 0)["n_comp"])


def test_operator_cases_are_what_they_claim():
    c = CC.operator_cases()
    n = lambda name, conn: CC.components(CC.pack(c[name]), *c[name].shape[1:], conn, 1, 0)["n_comp"].tolist()
    assert n("one_word", 4) == n("one_word", 8) == [0, 1, 1, 16]
    assert n("seams", 8) == [3, 1] and n("seams", 4) == [3, 1]
    assert n("diagonal", 4) == [2, 2] and n("diagonal", 8) == [1, 1]
    assert n("diagonal_seam", 4) == [2, 2] and n("diagonal_seam", 8) == [1, 1]
    assert n("board_and_u", 4) == [512, 1] and n("board_and_u", 8) == [1, 1]
    assert n("serpentine_squares_three", 4) == [1, 2, 3]
    two = CC.components(CC.pack(c["serpentine_squares_three"][1:2]), 64, 64, 8, 2, 0)["comps"][0]
    assert two[0].tolist() == [25, 4, 3, 8, 7, 3 * 64 + 4] and two[1].tolist() == [25, 50, 40, 54, 44, 40 * 64 + 50]


def test_min_area_one_reproduces_the_plane():
    planes = CC.operator_cases()["random"]
    P, H, W = planes.shape
    bits = CC.pack(planes)
    got = host_components(bits, H, W, 4, 1, 1)
    area, box = XO.stats(planes)
    assert np.array_equal(got["kept_bits"], bits) and np.array_equal(got["kept_area"], area) and np.array_equal(got["kept_box"], box)
    assert np.array_equal(got["n_kept"], got["n_comp"])


@pytest.fixture(scope="module")
def ref_bits(golden_dir):
    with np.load(os.path.join(golden_dir, "demo_classes_digest.npz")) as z:
        bits = z["mask_bits"]
    return np.ascontiguousarray(bits.reshape(-1, bits.shape[-1]))


def test_host_entry_equals_oracle_on_the_reference_planes(ref_bits):
    S = spec.DEMO_SAM.inp_size
    assert ref_bits.shape == (6, S * S // 8)
    for conn in (4, 8):
        want = CC.components(ref_bits, S, S, conn, 5, 64)
        assert_equal(host_components(ref_bits, S, S, conn, 5, 64), want, conn)
        print(f"reference planes, connectivity {conn}: n_comp {want['n_comp'].tolist()} largest {want['comps'][:, 0, 0].tolist()} "
              f"kept at 64 {want['n_kept'].tolist()} kept area {want['kept_area'].tolist()}")
        # the fixture is not degenerate: thousands of regions, a unique largest one, a few hundred of 64 pixels or more
        assert (want["comps"][:, 0, 0] > want["comps"][:, 1, 0]).all()
        assert want["kept_area"].min() > 0 and (want["kept_area"] < XO.stats(XO.unpack(ref_bits, S, S))[0]).all()
        assert 8380 <= want["n_comp"].min() and want["n_comp"].max() <= 9600
        assert 365 <= want["n_kept"].min() and want["n_kept"].max() <= 856


# ---- the entries refuse before they touch anything --------------------------------------------------------------------------------------
def test_mask_components_refuses_bad_arguments_without_gpu():
    lib = hip.load()
    p = 4096
    ok = dict(bits=p, P=2, H=4, W=64, conn=8, M=3, min_area=2, ws=p, ws_bytes=14 * 4 * 64, n_comp=p, comps=p, n_kept=p, kept_bits=p,
              kept_area=p, kept_box=p)
    bad = [dict(bits=None), dict(n_comp=None), dict(bits=p + 2), dict(kept_bits=p + 2), dict(P=0), dict(P=-1), dict(P=65536), dict(H=0),
           dict(H=-4), dict(W=0), dict(W=-64), dict(W=48), dict(W=8), dict(H=2 ** 16, W=2 ** 15), dict(H=2 ** 20, W=2 ** 20),
           dict(conn=6), dict(conn=0), dict(conn=-8), dict(M=-1), dict(M=65), dict(M=0), dict(comps=None), dict(min_area=-1),
           dict(min_area=0), dict(n_kept=None), dict(kept_bits=None), dict(kept_area=None), dict(kept_box=None)]

    def device(**kw):
        a = dict(ok, **kw)
        return lib.cvlm_mask_components(a["bits"], a["P"], a["H"], a["W"], a["conn"], a["M"], a["min_area"], a["ws"], a["ws_bytes"],
                                        a["n_comp"], a["comps"], a["n_kept"], a["kept_bits"], a["kept_area"], a["kept_box"], None)

    def host(**kw):
        a = dict(ok, **kw)
        return lib.cvlm_debug_mask_components_host(a["bits"], a["P"], a["H"], a["W"], a["conn"], a["M"], a["min_area"], a["n_comp"],
                                                   a["comps"], a["n_kept"], a["kept_bits"], a["kept_area"], a["kept_box"])
    for kw in bad:
        assert device(**kw) == -1, kw
        assert host(**kw) == -1, kw
    for kw in (dict(ws=None), dict(ws=p + 8), dict(ws_bytes=14 * 4 * 64 - 1), dict(ws_bytes=0), dict(ws_bytes=-1)):
        assert device(**kw) == -1, kw
    assert device(M=0, comps=None, min_area=0, n_kept=None, kept_bits=None, kept_area=None, kept_box=None, ws=None) == -1
    size = lib.cvlm_mask_components_workspace_bytes
    assert size(1, 4, 64) == 14 * 4 * 64 and size(7, 32, 64) == 7 * 14 * 32 * 64 and size(65535, 1024, 1024) == 65535 * 14 * 2 ** 20
    for P, H, W in ((0, 4, 64), (65536, 4, 64), (1, 0, 64), (1, 4, 0), (1, 4, 48), (1, -4, 64), (1, 2 ** 16, 2 ** 15)):
        assert size(P, H, W) == -1, (P, H, W)
    with pytest.raises(RuntimeError):
        hip.mask_components_workspace_bytes(1, 4, 48)


# ---- the host request -----------------------------------------------------------------------------------------------------------------------
def test_components_request_accepts_and_refuses():
    assert components_request(masks="logits") == (False, 0, 0, 8)                 # the default: nothing asked for
    assert components_request(masks="bits") == (False, 0, 0, 8)
    assert components_request(components=4, min_area=16, masks="bits") == (True, 4, 16, 8)
    assert components_request(components=0, masks="both", connectivity=4) == (True, 0, 0, 4)
    assert components_request(components=64, masks="bits") == (True, 64, 0, 8)
    assert components_request(min_area=1, masks="bits") == (True, 0, 1, 8)
    assert components_request(components=np.int64(3), min_area=np.int32(2), masks="both") == (True, 3, 2, 8)
    bad = [dict(components=-1), dict(components=65), dict(components=1.0), dict(components="1"), dict(components=True),
           dict(min_area=-1), dict(min_area=1.5), dict(min_area=None), dict(min_area=True),
           dict(components=1, masks="logits"), dict(min_area=1, masks="logits"), dict(components=0, masks="logits"),
           dict(components=1, connectivity=6), dict(connectivity=6), dict(connectivity="8"), dict(connectivity=True), dict(connectivity=None)]
    for kw in bad:
        with pytest.raises(ValueError):
            components_request(**dict(dict(masks="bits"), **kw))
    with pytest.raises(ValueError, match="infer_classes"):
        components_request(components=99, masks="bits", who="infer_classes")


def test_class_hypotheses_component_fields_are_optional():
    t = torch.zeros(1)
    h = ClassHypotheses(classes=t, pass1_logits=t, masks=t, edges=t, logits=t, pred=t)
    names = ("n_comp", "comps", "n_kept", "kept_bits", "kept_area", "kept_box")
    assert all(getattr(h, n) is None for n in names)
    assert [f.name for f in dataclasses.fields(h)] == ["classes", "pass1_logits", "masks", "edges", "logits", "pred"]
    h = ClassHypotheses(classes=t, pass1_logits=t, masks=None, edges=None, logits=t, pred=t, mask_bits=t, **{n: t for n in names})
    assert all(getattr(h, n) is t for n in names) and h.inter is None
