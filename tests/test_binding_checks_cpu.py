"""What the Python binding of the packed-mask entries refuses before anything is launched (camouflaged_vlm_amd/hip.py): one valid argument set
per launcher at the smallest shapes that still tell its arguments apart, and every tensor argument in turn with a wrong dtype, on another device
(a `meta` tensor), one row too many, a strided view, or -- for arguments that come together or not at all -- one member missing.  `hip._call` is replaced by a recorder,
so nothing in the library runs."""
import pytest
import torch

i16, i32, i64, u8, f32, f64 = torch.int16, torch.int32, torch.int64, torch.uint8, torch.float32, torch.float64


def z(dtype, *shape):
    return torch.zeros(shape, dtype=dtype)


def sized(prefix: str = "", offsets: str = "offsets"):
    """Two planes of 1 x 1 and 3 x 33 (a row crosses a 32-bit word): 4 and 24 bytes."""
    return {prefix + "bits": z(u8, 28), prefix + offsets: torch.tensor([0, 4, 28]), prefix + "dims": torch.tensor([[1, 1], [3, 33]], dtype=i32)}


def coco(boundary: bool):
    """E = 2 groups of one detection and one annotation: N = ND = NG = 2; T = 2 thresholds, A = 1 range."""
    a = dict(det_offsets=torch.tensor([0, 1, 2], dtype=i32), gt_offsets=torch.tensor([0, 1, 2], dtype=i32), pair_offsets=torch.tensor([0, 1, 2]),
             inter=z(i32, 2), det_area=z(i32, 2), score=z(f32, 2), gt_area=z(i32, 2), gt_range_area=z(f64, 2), gt_crowd=z(u8, 2),
             iou_thrs=z(f64, 2), area_rngs=z(f64, 1, 2), max_det=100)
    if boundary:
        a.update(inter_b=z(i32, 2), det_area_b=z(i32, 2), gt_area_b=z(i32, 2))
    a.update(dt_order=z(i32, 2), dt_match=z(i32, 1, 2, 2), dt_ignore=z(u8, 1, 2, 2), gt_match=z(i32, 1, 2, 2), gt_ignore=z(u8, 1, 2), status=z(i32, 1))
    return a


def groups():
    """G = 2 groups of one plane each over the sized table: no pairs, so inter has the one entry a launch needs."""
    return dict(group_offsets=torch.tensor([0, 1, 2], dtype=i32), member=z(i32, 2), pair_offsets=z(i64, 3), inter=z(i32, 2))


def label_state(score=True, ids=True):
    """B = 2 images of 1 x 1 and 2 x 3 (7 pixels), K = 2 hypotheses."""
    a = dict(score=z(f32, 7)) if score else {}
    a.update(winner=z(i16, 7), segment=z(i16, 7), areas=z(i32, 3, 4))
    if ids:
        a.update(segment_id=z(i32, 4), n_segments=z(i32, 2))
    return dict(a, status=z(i32, 1))


def pixels():
    return dict(dims=torch.tensor([[1, 1], [2, 3]], dtype=i32), pix_offsets=torch.tensor([0, 1, 7]))


FIXED = dict(bits=z(u8, 2, 128), H=32, W=32)
KEPT, FILLED, AREA_BOX = ("n_kept", "kept_bits", "kept_area", "kept_box"), ("n_filled", "filled_bits", "filled_area"), ("area", "box")
RLE = dict(offsets=torch.tensor([0, 1, 2]), counts=z(i32, 2), status=z(i32, 1))
RINGS = dict(vertex_offsets=torch.tensor([0, 4, 8]), xy=z(i16, 8, 2), ring_start=z(u8, 8), n_rings=z(i32, 2, 2))

# (launcher, whether it is a host form, symbol, arguments, groups given together or not at all, tensors whose number of rows is free: a flat
# tensor of any length, or the one tensor that a count is read from)
LAUNCHERS = []


def pair(name, args, together=(), free=(), device_only=(), host=None, symbol=None):
    """A device launcher `name` and its host twin `name`_host (or `host`)."""
    symbol = symbol or "cvlm_" + name
    LAUNCHERS.append((name, False, symbol, args, together, free))
    LAUNCHERS.append((host or name + "_host", True, "cvlm_debug_" + symbol[5:] + "_host", {k: v for k, v in args.items() if k not in device_only},
                      together, free))


def flagged(name, args, together=(), free=()):
    """A launcher with `host: bool`."""
    for host in (False, True):
        LAUNCHERS.append((name, host, "cvlm_debug_" + name + "_host" if host else "cvlm_" + name, dict(args, host=host), together, free))


pair("mask_components", dict(FIXED, connectivity=8, min_area=1, workspace=z(u8, 64), n_comp=z(i32, 2), comps=z(i32, 2, 2, 6), n_kept=z(i32, 2),
                             kept_bits=z(u8, 2, 128), kept_area=z(i32, 2), kept_box=z(i32, 2, 4)), (KEPT,), ("workspace",), ("workspace",))
pair("mask_holes", dict(FIXED, connectivity=8, fill_below=1, workspace=z(u8, 64), n_holes=z(i32, 2), holes=z(i32, 2, 2, 6), n_filled=z(i32, 2),
                        filled_bits=z(u8, 2, 128), filled_area=z(i32, 2)), (FILLED,), ("workspace",), ("workspace",))
pair("mask_morph", dict(FIXED, radius=1, dil_bits=z(u8, 2, 128), dil_area=z(i32, 2), ero_bits=z(u8, 2, 128), ero_area=z(i32, 2),
                        band_bits=z(u8, 2, 128), band_area=z(i32, 2)), (("dil_bits", "dil_area"), ("ero_bits", "ero_area"), ("band_bits", "band_area")))
pair("edge_pack", dict(prob=z(f32, 2, 3, 5), hout=32, wout=32, threshold=0.5, bits=z(u8, 2, 128), area=z(i32, 2), with_bits=z(u8, 2, 128),
                       with_inter=z(i32, 2)), (("with_bits", "with_inter"),))
LAUNCHERS += [
    ("mask_rle_count", False, "cvlm_mask_rle_count", dict(FIXED, n_runs=z(i32, 2)), (), ()),
    ("mask_rle_emit", False, "cvlm_mask_rle_emit", dict(FIXED, **RLE, workspace=z(u8, 64)), (), ("counts", "workspace")),
    ("mask_rle_host", True, "cvlm_debug_mask_rle_host", dict(FIXED, n_runs=z(i32, 2), **RLE), (("offsets", "counts", "status"),), ("counts",)),
    ("mask_rle_count_w", False, "cvlm_mask_rle_count_w", dict(FIXED, Wt=31, n_runs=z(i32, 2)), (), ()),
    ("mask_rle_emit_w", False, "cvlm_mask_rle_emit_w", dict(FIXED, Wt=31, **RLE, workspace=z(u8, 64)), (), ("counts", "workspace")),
    ("mask_rle_host_w", True, "cvlm_debug_mask_rle_host_w", dict(FIXED, Wt=31, n_runs=z(i32, 2), **RLE), (("offsets", "counts", "status"),), ("counts",)),
]
pair("mask_pack_sized", dict(logits=z(f32, 2, 3, 5), dims=sized()["dims"], offsets=sized()["offsets"], level=128, bits=z(u8, 28), max_words=6,
                             area=z(i32, 2), box=z(i32, 2, 4), status=z(i32, 1)), (AREA_BOX,), ("bits",))
pair("mask_rle_decode", dict(counts=z(i32, 4), run_offsets=torch.tensor([0, 2, 4]), **sized(offsets="bit_offsets"), max_pixels=99, area=z(i32, 2),
                             box=z(i32, 2, 4), status=z(i32, 1), workspace=z(u8, 64)), (AREA_BOX,), ("counts", "bits", "workspace"), ("workspace",))
pair("mask_poly_decode", dict(xy=z(f64, 12), poly_offsets=torch.tensor([0, 6, 12]), plane_polys=torch.tensor([0, 1, 2], dtype=i32),
                              **sized(offsets="bit_offsets"), max_pixels=99, area=z(i32, 2), box=z(i32, 2, 4), status=z(i32, 1), workspace=z(u8, 64)),
     (AREA_BOX,), ("xy", "poly_offsets", "bits", "workspace"), ("workspace",))
pair("mask_inter_sized", dict(**sized("a_"), **sized("b_"), pairs=z(i32, 2, 2), max_words=6, inter=z(i32, 2), status=z(i32, 1)), (),
     ("a_bits", "b_bits"))
pair("coco_match", coco(False), (), ("inter",))
pair("coco_match_boundary", coco(True))
pair("mask_boundary_sized", dict(sized(), radius=z(i32, 2), max_words=6, workspace=z(u8, 28), out_bits=z(u8, 28), out_area=z(i32, 2), status=z(i32, 1)))
LAUNCHERS += [
    ("mask_contour_count", False, "cvlm_mask_contour_count", dict(sized(), connectivity=8, max_words=6, n_vertices=z(i32, 2), status=z(i32, 1)), (),
     ("bits",)),
    ("mask_contour_emit", False, "cvlm_mask_contour_emit", dict(sized(), connectivity=8, max_words=6, **RINGS, round_vertices=8, status=z(i32, 1),
                                                                workspace=z(u8, 64)), (), ("bits", "workspace")),
    ("mask_contour_host", True, "cvlm_debug_mask_contour_host", dict(sized(), connectivity=8, n_vertices=z(i32, 2), status=z(i32, 1), **RINGS),
     (tuple(RINGS),), ("bits",)),
]
pair("mask_distance_sized", dict(sized(), reach=z(i32, 2), max_words=6, pix_offsets=torch.tensor([0, 1, 100]), workspace=z(u8, 208),
                                 out_d2=z(i32, 100), status=z(i32, 1)), (), ("bits", "workspace", "out_d2"))
pair("mask_surface_totals", dict(sized("a_"), b_d2=z(i32, 100), b_pix_offsets=torch.tensor([0, 1, 100]), b_dims=sized()["dims"], pairs=z(i32, 2, 2),
                                 radii=z(i32, 2, 2), max_words=6, workspace=z(u8, 64), n=z(i32, 2), far=z(i32, 2), within=z(i32, 2, 2),
                                 max_d2=z(i32, 2), sum_d2=z(i64, 2), sum_d=z(f64, 2), status=z(i32, 1)), (), ("a_bits", "b_d2", "workspace"))
pair("mask_thin_sized", dict(sized(), max_iter=z(i32, 2), max_words=6, mode=0, steps=4, workspace=z(u8, 64), out_bits=z(u8, 28), out_area=z(i32, 2),
                             out_box=z(i32, 2, 4), out_iters=z(i32, 2), out_done=z(i32, 2), status=z(i32, 1)), (("out_area", "out_box"),), ("workspace",))
pair("mask_regions_sized", dict(sized(), max_words=6, connectivity=8, min_area=1, workspace=z(u8, 64), n_regions=z(i32, 2), regions=z(i32, 2, 2, 6),
                                out_bits=z(u8, 56), status=z(i32, 1)), (), ("workspace",), ("workspace",))
pair("region_alpha", dict(sized(), alpha=z(f32, 2, 3, 3), src=z(i32, 2), out=z(f32, 2, 3, 3), status=z(i32, 1)), (), ("bits", "alpha"))
flagged("mask_nms_inter", dict(sized(), area=z(i32, 2), box=z(i32, 2, 4), **groups(), status=z(i32, 1)), (), ("bits", "inter"))
flagged("mask_nms", dict(groups(), area=z(i32, 2), score=z(f32, 2), category=z(i32, 2), measure=0, method=0, thr=0.5, sigma=0.5, order=z(i32, 2),
                         keep=z(u8, 2), by=z(i32, 2), decay=z(f32, 2), n_keep=z(i32, 2), status=z(i32, 1)), (), ("inter",))
flagged("render", dict(img=z(u8, 21), img_offsets=torch.tensor([0, 3, 21]), dims=torch.tensor([[1, 1], [2, 3]], dtype=i32), max_pixels=6,
                       layer_offsets=torch.tensor([0, 1, 1], dtype=i32), layers=z(i64, 1, 4), bits=z(u8, 28), levels=z(u8, 7), labels=z(i32, 7),
                       rgb=z(u8, 2, 3), alpha=z(f32, 2), out=z(u8, 21), status=z(i32, 1)), (), ("layers", "bits", "levels", "labels"))
flagged("label_init", dict(label_state(), B=2, K=2))
flagged("label_accumulate", dict(planes=z(f32, 2, 3, 5), p0=0, B=2, K=2, **pixels(), weights=z(f32, 4), level=128, max_pixels=6,
                                 **label_state(ids=False)), (), ("planes",))
flagged("label_finish", dict(B=2, K=2, **pixels(), overlap_threshold=0.5, max_pixels=6, **label_state(score=False)))
flagged("label_lookup", dict(map_=z(i16, 7), B=2, K=2, **pixels(), max_pixels=6, table=z(i32, 4), void=255, out=z(i32, 7), status=z(i32, 1)))
flagged("label_iou_hist", dict(pred=z(i32, 7), gt=z(i32, 7), num_classes=3, ignore_index=255, reduce_zero_label=False, zero_first=True,
                               totals=z(i64, 3, 3)))
flagged("pan_remap", dict(raw=z(i32, 7), B=2, **pixels(), max_pixels=6, keys=z(i32, 3), vals=z(i32, 3), table_offsets=torch.tensor([0, 1, 3]),
                          out=z(i32, 7), unknown=z(i32, 2), status=z(i32, 1)))
flagged("pan_pair_hist", dict(pred=z(i32, 7), gt=z(i32, 7), B=2, G=2, S=3, **pixels(), max_pixels=6, zero_first=True, inter=z(i32, 2, 2, 3),
                              status=z(i32, 1)))
flagged("pan_match", dict(inter=z(i32, 2, 2, 3), pred_cat=z(i32, 2, 3), gt_cat=z(i32, 2, 2), gt_crowd=z(u8, 2, 2), num_classes=3,
                          pred_match=z(i32, 2, 3), pred_iou=z(f64, 2, 3), gt_match=z(i32, 2, 2), pred_area=z(i32, 2, 3), gt_area=z(i32, 2, 2)))
flagged("pan_accumulate", dict(pred_cat=z(i32, 2, 3), gt_cat=z(i32, 2, 2), pred_match=z(i32, 2, 3), pred_iou=z(f64, 2, 3), gt_match=z(i32, 2, 2),
                               num_classes=3, zero_first=True, counts=z(i64, 3, 3), iou_sum=z(f64, 3)))


@pytest.fixture()
def hip(monkeypatch):
    from camouflaged_vlm_amd import hip
    hip.calls = []
    monkeypatch.setattr(hip, "_call", lambda name, *a: hip.calls.append(name))
    yield hip
    del hip.calls


def mutations(args, together, free):
    """(what, the arguments with one tensor spoiled) for every tensor argument in turn."""
    for name, t in args.items():
        if not isinstance(t, torch.Tensor):
            continue
        yield f"{name}: dtype", dict(args, **{name: t.to(torch.float16)})
        yield f"{name}: on another device", dict(args, **{name: t.to("meta")})
        if name not in free:
            yield f"{name}: one row too many", dict(args, **{name: torch.cat([t, t[:1]])})
        if t.numel() > 1:
            d = next(d for d in range(t.dim()) if t.shape[d] > 1)
            strided = torch.cat([t, t], dim=d)[(slice(None),) * d + (slice(None, None, 2),)]
            assert strided.shape == t.shape and not strided.is_contiguous()
            yield f"{name}: strided", dict(args, **{name: strided})
    for group in together:
        for name in group:
            yield f"{name}: missing from its group", dict(args, **{name: None})


IDS = [name + ("[host]" if host and not name.endswith(("_host", "_host_w")) else "") for name, host, *_ in LAUNCHERS]


@pytest.mark.parametrize("name, host, symbol, args, together, free", LAUNCHERS, ids=IDS)
def test_a_spoiled_tensor_is_refused_before_the_call(hip, name, host, symbol, args, together, free):
    """The valid set reaches the entry (the host forms) or the device check (the device forms: their tensors are host tensors here);
    every mutation is refused by an AssertionError before either."""
    fn = getattr(hip, name)
    if host:
        fn(**args)
        assert hip.calls == [symbol]
    else:
        with pytest.raises(RuntimeError):                   # _on_current_device: without a device its very message cannot be formed
            fn(**args)
        assert hip.calls == []
    hip.calls.clear()
    accepted = []
    for what, bad in mutations(args, together, free):
        try:
            fn(**bad)
            accepted.append(what)
        except AssertionError:
            pass
        except Exception as e:                              # noqa: BLE001 -- any other error is reported with the mutation that raised it
            accepted.append(f"{what} -> {type(e).__name__}")
    assert accepted == [] and hip.calls == []


def test_the_table_holds_every_launcher_with_a_host_form(hip):
    names = {name for name, *_ in LAUNCHERS}
    public = {n for n in dir(hip) if n.endswith(("_host", "_host_w"))} | {n for n in ("mask_nms_inter", "mask_nms", "render")} | \
             {n for n in dir(hip) if n.startswith(("label_", "pan_")) and n != "pan_lds_cells"}
    assert public <= names, public - names


@pytest.mark.gpu
def test_device_launchers_refuse_host_tensors_and_host_forms_device_tensors(hip):
    for name, host, symbol, args, together, free in LAUNCHERS:
        if host:
            with pytest.raises(AssertionError):
                getattr(hip, name)(**{k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in args.items()})
        else:
            with pytest.raises(RuntimeError, match="current device"):
                getattr(hip, name)(**args)
        assert hip.calls == [], name
