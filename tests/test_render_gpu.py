"""Rendering on the device: cvlm_render == its host twin == the oracle (tests/render_oracle.py) byte for byte on the
ragged scene -- runs that straddle row and word ends, dirty pad bits, all three kinds -- and on all 65 536 (c, col) pairs at six
alphas, every output pre-filled with garbage between guard bands, a second call giving identical bytes; in place; refusals as on the
host; the tiny engine through pack_masks_sized(level=1) -> render_overlay against demo.py:51-56 restated in numpy, with outlines and
with a panoptic colour map; no layer launches nothing and bad arguments raise first."""
import os

import numpy as np
import pytest
import torch

import render_oracle as RO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from camouflaged_vlm_amd import hip
    hip.load()
    return hip


@pytest.fixture(scope="module")
def sc():
    return RO.scene()


def test_device_equals_host_twin_equals_oracle_on_the_scene(hip, sc):
    want = RO.render_oracle(sc)
    got = RO.run(hip, sc, dev=DEV)
    assert got["status"] == 0 and got["bands"]
    assert got["out"].tobytes() == want.tobytes()
    host = RO.run(hip, sc)
    assert host["status"] == 0 and got["out"].tobytes() == host["out"].tobytes()
    again = RO.run(hip, sc, dev=DEV)
    assert again["status"] == 0 and again["bands"] and again["out"].tobytes() == got["out"].tobytes()


@pytest.mark.parametrize("a", RO.ALPHAS)
def test_all_65536_pairs_on_the_device(hip, a):
    t = RO.table_scene(a)
    got = RO.run(hip, t, dev=DEV)
    assert got["status"] == 0 and got["bands"]
    assert got["out"].tobytes() == RO.render_oracle(t).tobytes()
    assert got["out"].tobytes() == RO.run(hip, t)["out"].tobytes()
    if a == 0.5:
        c, col = np.meshgrid(np.arange(256.0), np.arange(256.0), indexing="ij")
        assert np.array_equal(got["out"].reshape(256, 256, 3)[..., 0], np.rint((c + col) / 2).astype(np.uint8))
    assert RO.run(hip, t, dev=DEV)["out"].tobytes() == got["out"].tobytes()


def test_in_place_on_the_device(hip, sc):
    got = RO.run(hip, sc, dev=DEV, in_place=True)
    assert got["status"] == 0 and got["bands"]
    assert got["out"].tobytes() == RO.in_place_expected(sc).tobytes()
    t = RO.table_scene(0.3)
    assert RO.run(hip, t, dev=DEV, in_place=True)["out"].tobytes() == RO.in_place_expected(t).tobytes()


def test_refusals_on_the_device_are_the_host_twins(hip, sc):
    for name, over, status, skip, refused in RO.refusal_cases(sc):
        d, h = RO.run(hip, sc, dev=DEV, **over), RO.run(hip, sc, **over)
        assert d["status"] == h["status"] == status and d["bands"], (name, d["status"], h["status"])
        assert d["out"].tobytes() == h["out"].tobytes(), name
    t = sc["layers"].copy()
    t[0, 0] = 9
    a = sc["alpha"].copy()
    a[int(sc["layers"][-2, 2])] = np.nan                              # image 7's fill
    over = dict(layers=t, alpha=a, dims=np.concatenate([sc["dims"][:6], [[0, 37]], sc["dims"][7:]]).astype(np.int32))
    d, h = RO.run(hip, sc, dev=DEV, **over), RO.run(hip, sc, **over)
    assert d["status"] == h["status"] == 7 and d["out"].tobytes() == h["out"].tobytes() and d["bands"]
    d = RO.run(hip, sc, dev=DEV, in_place=True, **over)
    assert d["status"] == 7 and d["out"].tobytes() == RO.run(hip, sc, in_place=True, **over)["out"].tobytes()


# ---- the tiny engine -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, "tiny_classes.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def chain(gold):
    """The engine (the recipe of tests/test_nms_gpu.py), batch 2 with one hypothesis per image, the mask logits, two synthetic
    photographs at the ragged sizes (37, 45) and (50, 33) and the demo's `data_array > 0` planes at those sizes."""
    from camouflaged_vlm_amd import maskpost, spec, synth
    from camouflaged_vlm_amd.engine import Cascade, Precision
    g, c = spec.TINY_SAM, spec.TINY_CLIP
    dev = torch.device(DEV)
    sd_np = synth.make_full_state_dict(g, c)
    inp, ci, cm = (torch.from_numpy(t).to(dev) for t in synth.make_inputs(g, c, batch=2))
    cas = Cascade({k: torch.from_numpy(v) for k, v in sd_np.items()}, g, c, dev, Precision.named("exact"))
    cas.clip.set_text_bank(cas.clip.text_features(gold["eot_test"].tolist(), "test"), torch.from_numpy(gold["bank_test"]), "test")
    h = cas.infer_classes(inp, ci, cm, topk=1)
    logits = h.masks.reshape(-1, 1, g.inp_size, g.inp_size).clone()
    sizes = [(37, 45), (50, 33)]
    rng = np.random.default_rng(11)
    photos = [rng.integers(0, 256, (hh, ww, 3), dtype=np.uint8) for hh, ww in sizes]
    images = maskpost.sized_images([photos[0], torch.from_numpy(photos[1]).to(dev)], dev)       # one from the host, one from the device
    sized = cas.pack_masks_sized(logits, sizes, level=1)
    return dict(cas=cas, logits=logits, sizes=sizes, photos=photos, images=images, sized=sized)


def test_the_demo_picture_from_the_engine(chain):
    cas, images, sized, photos = chain["cas"], chain["images"], chain["sized"], chain["photos"]
    for b in range(2):
        assert np.array_equal(images.to_numpy(b), photos[b])
    out = cas.render_overlay(images, sized, image_of=range(2))
    out.check()
    masks = [sized.to_numpy(p) for p in range(2)]
    print(f"demo overlay: {[int(m.sum()) for m in masks]} masked pixels of {[m.size for m in masks]}")
    assert all(0 < int(m.sum()) for m in masks)
    for b in range(2):
        assert np.array_equal(out.to_numpy(b), RO.demo_overlay(photos[b], masks[b]))
    assert out.sizes == images.sizes and out.data.data_ptr() != images.data.data_ptr()
    # with outlines: the boundary of radius 1 painted white at alpha 1 over the overlay
    lined = cas.render_overlay(images, sized, image_of=range(2), outline=1)
    lined.check()
    edges = cas.mask_boundary_sized(sized, radius=1)
    for b in range(2):
        want = RO.demo_overlay(photos[b], masks[b])
        e = edges.to_numpy(b)
        assert 0 < int(e.sum()) and not (e & ~masks[b]).any()
        want[e] = (255, 255, 255)
        assert np.array_equal(lined.to_numpy(b), want)


def test_a_panoptic_colour_map_from_the_engine(chain):
    from camouflaged_vlm_amd import maskpost
    cas, images, photos, sizes = chain["cas"], chain["images"], chain["photos"], chain["sizes"]
    maps = cas.label_maps(chain["logits"], sizes, K=1, level=1)
    pan = maps.panoptic()
    pal = maskpost.palette(8)
    layers = [[maskpost.classes(pan, maps, b, palette=pal, alpha=0.7), maskpost.classes(pan, maps, b, palette=pal[::-1].copy(), alpha=1.0, edges=True)]
              for b in range(2)]
    out = cas.render(images, layers)
    out.check()
    for b in range(2):
        ids = maps.image_of(pan, b).cpu().numpy()
        assert set(np.unique(ids).tolist()) <= {0, 1}
        want = RO.blend(photos[b], pal[ids], np.float32(0.7))
        e = RO.edges_of(ids)
        want[e] = pal[::-1][ids][e]
        assert np.array_equal(out.to_numpy(b), want)


def test_no_layer_launches_nothing_and_bad_arguments_raise_first(chain, monkeypatch):
    from camouflaged_vlm_amd import hip, maskpost
    cas, images, sized = chain["cas"], chain["images"], chain["sized"]
    calls = []
    monkeypatch.setattr(hip, "render", lambda *a, **k: calls.append("render"))
    monkeypatch.setattr(hip, "_call", lambda name, *a: calls.append(name))
    out = cas.render(images, [[], []])
    assert calls == [] and torch.equal(out.data, images.data) and out.data.data_ptr() != images.data.data_ptr()
    assert out.status.tolist() == [0] and out.sizes == images.sizes
    host_images = maskpost.sized_images(chain["photos"], "cpu")
    swapped = maskpost.SizedMasks(bits=sized.bits, offsets=sized.offsets, area=sized.area, box=sized.box, status=sized.status, sizes=sized.sizes[::-1])
    for call in (lambda: cas.render(images, [[]]), lambda: cas.render(host_images, [[], []]), lambda: cas.render(images.data, [[], []]),
                 lambda: cas.render(images, [[maskpost.fill(sized, 1, color=(0, 255, 0))], []]),              # the plane of the other size
                 lambda: cas.render(images, [[maskpost.fill(host_sized(sized), 0, color=(0, 255, 0))], []]),  # a source on the host
                 lambda: cas.render_overlay(images, sized, image_of=[0]), lambda: cas.render_overlay(images, sized, image_of=[0, 2]),
                 lambda: cas.render_overlay(images, sized, image_of=[1, 0], outline=1), lambda: cas.render_overlay(images, sized, image_of=[0, 1], alpha=2.0),
                 lambda: cas.render_overlay(images, sized, image_of=[0, 1], colors=(0, 256, 0)),
                 lambda: cas.render_overlay(images, sized, image_of=[0, 1], outline=1, outline_color=(0, -1, 0)),
                 lambda: cas.render_overlay(images, sized, image_of=[0, 1], outline=0),
                 lambda: cas.render_overlay(images, swapped, image_of=[0, 1], outline=1)):
        with pytest.raises(ValueError):
            call()
    assert calls == []
    cas.render_overlay(images, sized, image_of=[0, 1])
    assert calls == ["render"]


def host_sized(sized):
    from camouflaged_vlm_amd import maskpost
    return maskpost.SizedMasks(bits=sized.bits.cpu(), offsets=sized.offsets.cpu(), area=None, box=None, status=sized.status.cpu(), sizes=sized.sizes)
