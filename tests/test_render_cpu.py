"""CPU: rendering -- cvlm_debug_render_host, the kernel's per-pixel functions (csrc/render_logic.h) run sequentially,
against the numpy oracle (tests/render_oracle.py): the ragged scene byte for byte, all 65 536 (c, col) pairs at six alphas, demo.py:51-56
restated, in place, every status refusal, every CVLM_E_BADARG with host pointers, every ValueError of render_request, the palette."""
import ctypes

import numpy as np
import pytest
import torch

import render_oracle as RO

@pytest.fixture(scope="module")
def hip():
    from camouflaged_vlm_amd import hip
    hip.load()
    return hip


@pytest.fixture(scope="module")
def sc():
    return RO.scene()


@pytest.fixture(scope="module")
def want(sc):
    return RO.render_oracle(sc)


def test_abi_stays_12_and_the_entries_are_bound(hip):
    lib = hip.load()
    assert lib.cvlm_abi_version() == hip.ABI_VERSION == 12
    for name in ("cvlm_render", "cvlm_debug_render_host"):
        assert name in hip.EXPORTS and hasattr(lib, name) and hip.ABI[name][0] is ctypes.c_int32
    assert hip._SIGNATURES["cvlm_render"] == hip._SIGNATURES["cvlm_debug_render_host"] + "s"


def test_the_scene_holds_what_the_design_lists(sc, want):
    assert sc["sizes"] == [(1, 1), (2, 3), (7, 5), (3, 31), (2, 32), (5, 33), (4, 37), (3, 65)]
    per = np.diff(sc["layer_offsets"]).tolist()
    assert per[1] == 0 and per[2] == 4
    kinds = [(int(r[0]) & 0xff, int(r[0]) >> 8) for r in sc["layers"]]
    lo, hi = sc["layer_offsets"][2:4]
    assert {k for k, _ in kinds[lo:hi]} == {0, 1, 2} and (0, RO.INVERT) in kinds[lo:hi] and (2, RO.EDGES) in kinds[lo:hi]
    assert bool((sc["alpha"] == 0).any()) and bool((sc["alpha"] == 1).any())
    for (kf, src, first, rows), b in zip(sc["layers"], np.repeat(np.arange(8), per)):
        h, w = sc["sizes"][b]
        if kf & 0xff == RO.BITS:                                      # every pad bit of every plane is 1
            ws = (w + 31) // 32
            rows_ = np.unpackbits(sc["bits"][src:src + 4 * h * ws].reshape(h, 4 * ws), axis=1)
            assert bool(rows_[:, w:].all())
        if kf == RO.LABELS | RO.EDGES << 8:                          # EDGES pixels lie on all four borders
            ids = sc["labels"][src:src + h * w].reshape(h, w)
            e = RO.edges_of(ids) & (ids >= 0) & (ids < rows)
            assert e[0].any() and e[-1].any() and e[:, 0].any() and e[:, -1].any()
    assert {-1, 2 ** 31 - 1} <= set(sc["labels"].tolist())
    # the two fills of image 3: the other order gives another picture
    a, b = int(sc["layer_offsets"][3]), int(sc["layer_offsets"][3]) + 1
    swapped = dict(sc, layers=sc["layers"].copy())
    swapped["layers"][[a, b]] = sc["layers"][[b, a]]
    assert not np.array_equal(RO.render_oracle(swapped), want)
    # and the oracle's blend rounds half to even and contracts nothing
    assert RO.blend(np.uint8(1), np.uint8(2), 0.5) == 2 and RO.blend(np.uint8(2), np.uint8(3), 0.5) == 2
    assert RO.blend(np.uint8(255), np.uint8(255), 1.0) == 255 and RO.blend(np.uint8(7), np.uint8(200), 0.0) == 7


def test_host_twin_equals_the_oracle(hip, sc, want):
    got = RO.run(hip, sc)
    assert got["status"] == 0 and got["bands"]
    assert got["out"].tobytes() == want.tobytes()                     # pad bytes included: they still hold the garbage
    again = RO.run(hip, sc)
    assert again["out"].tobytes() == got["out"].tobytes()


@pytest.mark.parametrize("a", RO.ALPHAS)
def test_all_65536_pairs(hip, a):
    t = RO.table_scene(a)
    got = RO.run(hip, t)
    assert got["status"] == 0 and got["bands"]
    assert got["out"].tobytes() == RO.render_oracle(t).tobytes()
    img = got["out"].reshape(256, 256, 3)
    c, col = np.meshgrid(np.arange(256.0), np.arange(256.0), indexing="ij")
    if a == 0.5:
        assert np.array_equal(img[..., 0], np.rint((c + col) / 2).astype(np.uint8))
        assert int((np.rint((c + col) / 2) != np.floor((c + col) / 2 + 0.5)).sum()) == 16384     # where half-up would differ
    if a in (0.0, 1.0):
        assert np.array_equal(img[..., 1], (c if a == 0.0 else col).astype(np.uint8))
    if a in (0.3, 0.7):                                               # a fused multiply-add would not pass: it changes some of these
        a32 = np.float32(a)
        b32 = np.float32(1.0) - a32
        p, q = (c.astype(np.float32) * b32).astype(np.float64), col * np.float64(a32)
        fused = np.clip(np.rint((p + q).astype(np.float32)), 0, 255).astype(np.uint8)     # c b rounded, col a kept exact: fma(col, a, c b)
        assert 100 <= int((fused != img[..., 2]).sum()) <= 200


def test_the_demo_restated(hip):
    from camouflaged_vlm_amd import maskpost
    rng = np.random.default_rng(5)
    h, w = 37, 45
    image = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    mask = rng.random((h, w)) < 0.4
    images = maskpost.sized_images([image], "cpu")
    assert images.sizes == [(h, w)] and np.array_equal(images.to_numpy(0), image) and tuple(images.image(0).shape) == (h, w, 3)
    dims, off, _ = maskpost.sized_tables([(h, w)])
    sized = maskpost.SizedMasks(bits=torch.from_numpy(RO.pack_rows(mask)), offsets=torch.from_numpy(off), area=None, box=None,
                                status=torch.zeros(1, dtype=torch.int32), sizes=[(h, w)], level=1)
    out = maskpost.MaskUtilities().render_overlay(images, sized, image_of=[0], host=True)
    out.check()
    assert np.array_equal(out.to_numpy(0), RO.demo_overlay(image, mask))
    assert np.array_equal(out.to_numpy(0)[~mask], image[~mask])       # what the mask does not select is the photograph
    # two planes in two colours on one image, and an image without a plane
    other = rng.random((h, w)) < 0.3
    both = maskpost.SizedMasks(bits=torch.from_numpy(np.concatenate([RO.pack_rows(mask), RO.pack_rows(other)])),
                               offsets=torch.from_numpy(maskpost.sized_tables([(h, w)] * 2)[1]), area=None, box=None,
                               status=torch.zeros(1, dtype=torch.int32), sizes=[(h, w)] * 2, level=1)
    two = maskpost.sized_images([image, image[:5, :7].copy()], "cpu")
    out = maskpost.MaskUtilities().render_overlay(two, both, image_of=[0, 0], colors=[(0, 255, 0), (255, 0, 0)], host=True)
    assert np.array_equal(out.to_numpy(0), RO.demo_overlay(RO.demo_overlay(image, mask), other, (255, 0, 0)))
    assert np.array_equal(out.to_numpy(1), image[:5, :7]) and int(out.status.item()) == 0


def test_in_place_gives_the_same_bytes(hip, sc, want):
    got = RO.run(hip, sc, in_place=True)
    assert got["status"] == 0 and got["bands"]
    assert got["out"].tobytes() == RO.in_place_expected(sc).tobytes()
    for b in range(len(sc["sizes"])):
        assert np.array_equal(RO.image_of(sc, got["out"], b), RO.image_of(sc, want, b))


def test_every_refusal_bit(hip, sc, want):
    for name, over, status, skip, refused in RO.refusal_cases(sc):
        got = RO.run(hip, sc, **over)
        assert got["status"] == status and got["bands"], (name, got["status"])
        assert got["out"].tobytes() == RO.render_oracle(sc, skip=skip, refused=refused).tobytes(), name      # as if absent; no byte written
    # a bad alpha in a LEVELS table: the pixels of that level alone stay, the others are painted; an unused bad row says nothing
    heat_l = next(l for l, r in enumerate(sc["layers"]) if int(r[0]) == RO.LEVELS)
    src, first = int(sc["layers"][heat_l, 1]), int(sc["layers"][heat_l, 2])
    used = int(sc["levels"][src])
    a = sc["alpha"].copy()
    a[first + used] = np.nan
    got = RO.run(hip, sc, alpha=a)
    zero = sc["alpha"].copy()
    zero[first + used] = 0.0                                          # paints nothing: what alpha 0 gives
    assert got["status"] == 4 and got["out"].tobytes() == RO.render_oracle(dict(sc, alpha=zero)).tobytes()
    spare = sc["alpha"].copy()
    spare[0] = np.nan                                                 # row 0 belongs to no layer
    got = RO.run(hip, sc, alpha=spare)
    assert got["status"] == 0 and got["out"].tobytes() == want.tobytes()
    # several at once: the bits are ORed
    t = sc["layers"].copy()
    t[0, 0] = 9
    got = RO.run(hip, sc, layers=t, dims=np.concatenate([sc["dims"][:7], [[0, 65]]]).astype(np.int32))
    assert got["status"] == 3 and got["out"].tobytes() == RO.render_oracle(sc, skip=(0,), refused=(7,)).tobytes()


def test_no_layer_is_a_copy(hip, sc):
    none = dict(layers=np.zeros((0, 4), np.int64), layer_offsets=np.zeros(9, np.int32))
    got = RO.run(hip, sc, **none)
    assert got["status"] == 0 and got["bands"] and got["out"].tobytes() == RO.render_oracle(dict(sc, **none)).tobytes()
    for b in range(8):
        assert np.array_equal(RO.image_of(sc, got["out"], b), RO.image_of(sc, sc["img"], b))


def test_every_badarg_with_host_pointers(hip, sc):
    lib = hip.load()
    t = {k: np.ascontiguousarray(v) for k, v in sc.items() if isinstance(v, np.ndarray)}
    B, L, T, n = len(sc["sizes"]), len(t["layers"]), len(t["alpha"]), t["img"].size
    out, status = np.zeros(n + 8, np.uint8), np.zeros(4, np.int32)
    p = lambda a, shift=0: a.ctypes.data + shift

    def call(**o):
        a = dict(img=p(t["img"]), img_bytes=n, img_offsets=p(t["img_offsets"]), dims=p(t["dims"]), B=B, max_pixels=sc["max_pixels"],
                 layer_offsets=p(t["layer_offsets"]), layers=p(t["layers"]), L=L, bits=p(t["bits"]), bits_bytes=t["bits"].size,
                 levels=p(t["levels"]), levels_bytes=t["levels"].size, labels=p(t["labels"]), labels_n=t["labels"].size, rgb=p(t["rgb"]),
                 alpha=p(t["alpha"]), T=T, out=p(out), status=p(status))
        a.update(o)
        return lib.cvlm_debug_render_host(*a.values())

    assert call() == 0 and status[0] == 0 and out[:n].tobytes() != bytes(n)
    assert call(bits=None, levels=None, labels=None) == 0 and status[0] == 2
    assert call(L=0, layers=None, layer_offsets=p(np.zeros(B + 1, np.int32))) == 0 and status[0] == 0
    own = t["img"].copy()
    assert call(img=p(own), out=p(own)) == 0                          # in place: exactly img
    for name in ("img", "img_offsets", "dims", "layer_offsets", "layers", "rgb", "alpha", "out", "status"):
        assert call(**{name: None}) == -1, name
    for name in ("img", "dims", "layer_offsets", "bits", "labels", "alpha", "out", "status"):
        assert call(**{name: p(np.zeros(4096, np.int32), 2)}) == -1, name
    for name in ("img_offsets", "layers"):
        assert call(**{name: p(np.zeros(4096, np.int64), 4)}) == -1, name
    big = np.zeros(n + 16, np.uint8)
    for o in (dict(B=0), dict(B=(1 << 16) + 1), dict(L=-1), dict(L=(1 << 20) + 1), dict(T=0), dict(T=(1 << 24) + 1), dict(img_bytes=3),
              dict(img_bytes=-1), dict(bits_bytes=-1), dict(levels_bytes=-1), dict(labels_n=-1), dict(max_pixels=0),
              dict(max_pixels=(1 << 28) + 1),
              dict(img=p(big), out=p(big, 4)), dict(img=p(big, 4), out=p(big)),        # out shares bytes with img without being img
              dict(out=p(t["bits"])), dict(out=p(t["levels"])), dict(out=p(t["labels"])), dict(out=p(t["rgb"])), dict(out=p(t["alpha"])),
              dict(out=p(t["layers"])), dict(out=p(t["img_offsets"])), dict(out=p(t["dims"])), dict(out=p(t["layer_offsets"])),
              dict(status=p(out, 4)), dict(status=p(t["img"], 4)), dict(status=p(t["alpha"])), dict(status=p(t["labels"])),
              dict(status=p(t["layers"], 8)), dict(status=p(t["dims"]))):
        assert call(**o) == -1, o


def test_palette():
    from camouflaged_vlm_amd import maskpost
    pal = maskpost.palette(256)
    assert pal.dtype == np.uint8 and pal.shape == (256, 3)
    assert pal[:5].tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128]]
    assert pal[15].tolist() == [192, 128, 128] and pal[255].tolist() == [224, 224, 192]
    assert len({tuple(r) for r in pal.tolist()}) == 256 and np.array_equal(maskpost.palette(7), pal[:7])
    assert np.array_equal(maskpost.palette(300)[256:], pal[:44])
    for bad in (0, -1, True, 2.0, "3", (1 << 24) + 1):
        with pytest.raises(ValueError):
            maskpost.palette(bad)


def test_render_request_raises_before_anything_is_launched(hip, monkeypatch):
    from camouflaged_vlm_amd import maskpost
    calls = []
    monkeypatch.setattr(hip, "_call", lambda name, *a: calls.append(name))
    h, w = 6, 40
    sizes = [(h, w), (3, 3)]
    off = maskpost.sized_tables([(h, w), (3, 3)])[1]
    sized = maskpost.SizedMasks(bits=torch.zeros(int(off[-1]), dtype=torch.uint8), offsets=torch.from_numpy(off), area=None, box=None,
                                status=torch.zeros(1, dtype=torch.int32), sizes=sizes)
    levels = torch.zeros(2, h, w, dtype=torch.uint8)

    class Maps:
        pass
    maps = Maps()
    maps.sizes = sizes
    label_map = torch.zeros(h * w + 9, dtype=torch.int32)
    lut = np.zeros((256, 3), np.int64)
    ok = [[maskpost.fill(sized, 0, color=(1, 2, 3)), maskpost.heat(levels, 1, lut=lut, alpha=0.5),
           maskpost.classes(label_map, maps, 0, palette=maskpost.palette(4), edges=True)], [maskpost.fill(sized, 1, color=[0, 0, 0], alpha=1, invert=True)]]
    req = maskpost.render_request(sizes, ok)
    assert req.L == 4 and req.layer_offsets.tolist() == [0, 3, 4] and req.rgb.shape == (1 + 256 + 4 + 1, 3) and req.alpha.dtype == np.float32
    assert req.layers[:, 0].tolist() == [0, 1, 2 | 1 << 8, 0 | 2 << 8] and req.layers[:, 3].tolist() == [1, 256, 4, 1]
    assert req.layers[:, 1].tolist() == [0, h * w, 0, int(off[1])] and req.layers[:, 2].tolist() == [0, 1, 257, 261]
    # two different bit sources: the second is shifted behind the first
    other = maskpost.SizedMasks(bits=torch.zeros(int(off[1]), dtype=torch.uint8), offsets=torch.from_numpy(off[:2]), area=None, box=None,
                                status=torch.zeros(1, dtype=torch.int32), sizes=sizes[:1])
    req2 = maskpost.render_request(sizes, [[maskpost.fill(sized, 0, color=(1, 2, 3)), maskpost.fill(other, 0, color=(1, 2, 3))], []])
    assert req2.layers[:, 1].tolist() == [0, int(off[-1])] and len(req2.sources[0]) == 2
    bad_layers = [
        lambda: maskpost.fill(sized, 2, color=(1, 2, 3)),                                   # no such plane
        lambda: maskpost.fill(sized, True, color=(1, 2, 3)),
        lambda: maskpost.fill(sized.bits, 0, color=(1, 2, 3)),
        lambda: maskpost.fill(sized, 0, color=(1, 2, 256)),
        lambda: maskpost.fill(sized, 0, color=(1, 2, -1)),
        lambda: maskpost.fill(sized, 0, color=(1.0, 2.0, 3.0)),
        lambda: maskpost.fill(sized, 0, color=(1, 2)),
        lambda: maskpost.fill(sized, 0, color=(1, 2, 3), alpha=float("nan")),
        lambda: maskpost.fill(sized, 0, color=(1, 2, 3), alpha=1.5),
        lambda: maskpost.fill(sized, 0, color=(1, 2, 3), alpha=-0.1),
        lambda: maskpost.fill(sized, 0, color=(1, 2, 3), alpha=True),
        lambda: maskpost.fill(sized, 0, color=(1, 2, 3), invert=1),
        lambda: maskpost.heat(levels, 2, lut=lut, alpha=0.5),
        lambda: maskpost.heat(levels.float(), 0, lut=lut, alpha=0.5),
        lambda: maskpost.heat(levels, 0, lut=lut[:255], alpha=0.5),
        lambda: maskpost.heat(levels, 0, lut=lut, alpha=np.zeros(255)),
        lambda: maskpost.heat(levels, 0, lut=lut, alpha=np.full(256, np.inf)),
        lambda: maskpost.classes(label_map, maps, 2, palette=maskpost.palette(4)),
        lambda: maskpost.classes(label_map.long(), maps, 0, palette=maskpost.palette(4)),
        lambda: maskpost.classes(label_map[:-1], maps, 0, palette=maskpost.palette(4)),
        lambda: maskpost.classes(label_map, maps, 0, palette=np.zeros((0, 3), np.uint8)),
        lambda: maskpost.classes(label_map, maps, 0, palette=np.zeros((4, 4), np.uint8)),
        lambda: maskpost.classes(label_map, maps, 0, palette=maskpost.palette(4), alpha=[0.5] * 3),
        lambda: maskpost.classes(label_map, sized.bits, 0, palette=maskpost.palette(4)),
    ]
    for make in bad_layers:
        with pytest.raises(ValueError):
            make()
    good = ok[0][0]
    import dataclasses
    for layers in (ok[:1], ok + [[]], [ok[1], ok[0]],                                       # the count; planes of the other image's size
                   [[good], good], [good, []], "ab", [["x"], []],
                   [[dataclasses.replace(good, alpha=np.float32([2.0]))], []], [[dataclasses.replace(good, rgb=np.asarray([[0, 0, 300]]))], []],
                   [[dataclasses.replace(good, flags=1)], []], [[dataclasses.replace(good, src=2)], []],
                   [[dataclasses.replace(good, src=int(off[-1]))], []], [[dataclasses.replace(good, kind=3)], []],
                   [[dataclasses.replace(ok[0][1], rgb=np.zeros((255, 3), np.uint8), alpha=np.zeros(255, np.float32))], []],
                   [[dataclasses.replace(ok[0][1], flags=2)], []], [[dataclasses.replace(ok[0][2], source=label_map.long())], []]):
        with pytest.raises(ValueError):
            maskpost.render_request(sizes, layers)
    for bad_sizes in ([], [(0, 3), (3, 3)], [(h, w)], "ab"):
        with pytest.raises(ValueError):
            maskpost.render_request(bad_sizes, ok)
    with pytest.raises(ValueError):
        maskpost.render_request(sizes, ok, device="cuda:0")           # the sources live on the host
    mu = maskpost.MaskUtilities()
    images = maskpost.sized_images([np.zeros((h, w, 3), np.uint8), np.zeros((3, 3, 3), np.uint8)], "cpu")
    for call in (lambda: mu.render(images, ok), lambda: mu.render(images.data, ok, host=True), lambda: mu.render(images, ok[:1], host=True),
                 lambda: mu.render_overlay(images, sized, image_of=[0], host=True), lambda: mu.render_overlay(images, sized, image_of=[1, 0], host=True),
                 lambda: mu.render_overlay(images, sized, image_of=[0, 2], host=True),
                 lambda: mu.render_overlay(images, sized, image_of=[0, 1], colors=[(1, 2, 3)] * 3, host=True),
                 lambda: mu.render_overlay(images, sized, image_of=[0, 1], outline=1, host=True),
                 lambda: maskpost.sized_images([np.zeros((3, 3), np.uint8)], "cpu"), lambda: maskpost.sized_images([], "cpu"),
                 lambda: maskpost.sized_images([np.zeros((3, 3, 3), np.float32)], "cpu"), lambda: maskpost.sized_images(np.zeros((1, 3, 3, 3), np.uint8), "cpu")):
        with pytest.raises(ValueError):
            call()
    assert calls == []
    # no layer for any image: a clone, nothing launched
    out = mu.render(images, [[], []], host=True)
    assert calls == [] and torch.equal(out.data, images.data) and out.data.data_ptr() != images.data.data_ptr() and int(out.status.item()) == 0
    out.check()
    mu.render(images, ok, host=True)
    assert calls == ["cvlm_debug_render_host"]
