"""Post-processing of mask hypotheses on the device: packed masks with areas, boxes and overlaps, connected
components, holes, the edge band, packed edge maps, COCO run-length encoding, masks at each image's own size, their intersections
with ground truth and COCO's matching of detections to annotations, label maps, panoptic quality, boundaries, contours and their
simplification, distance maps, thinning, regions, mask NMS and rendering.  Three layers: the pure host checks of every argument
(`*_request`) with the result types; `MaskUtilities`, the stand-alone utilities, which Cascade inherits; and `MaskPost`, the plan
of these outputs for one Cascade.infer_classes / decode call.  All three are written in the few private helpers at the top of the file: what an
int, a real and a sequence are, the one check of an (h, w) list, of "one int or one per plane", of the connectivity and of a
SizedMasks argument, the one upload, allocator and workspace rule.  `engine` imports every public name back: callers keep importing
them from there.  Kernels are called as `hip.<name>(...)`, looked up at call time, so that a test can stand in for a launch."""
from __future__ import annotations

from dataclasses import InitVar, dataclass
from functools import partial
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip


# ---- what every check, table and allocation below is made of ---------------------------------------------------------
def _is_int(v) -> bool:
    """An int, Python's or numpy's; a bool is none."""
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _is_real(v) -> bool:
    """An int or a float, Python's or numpy's; a bool is none."""
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def _is_seq(v) -> bool:
    """Something with a length that is no string."""
    return not isinstance(v, (str, bytes)) and hasattr(v, "__len__")


def _int_in(who: str, name: str, v, lo: int, hi: Optional[int] = None, none: bool = False) -> int:
    """v as an int in [lo, hi] (hi None: at least lo), no bool (ValueError otherwise); none=True only words the message for a caller
    that has taken None out before."""
    if not _is_int(v) or int(v) < lo or (hi is not None and int(v) > hi):
        raise ValueError(f"{who}: {name} must be {'None or ' if none else ''}an int {f'>= {lo}' if hi is None else f'in [{lo}, {hi}]'}, got {v!r}")
    return int(v)


def _connectivity(who: str, v) -> int:
    if not _is_int(v) or int(v) not in (4, 8):
        raise ValueError(f"{who}: connectivity must be the int 4 or 8, got {v!r}")
    return int(v)


def _int_list(who: str, name: str, seq, n: int, per: str = "plane") -> list:
    """n ints, no bools -> the list as ints (ValueError otherwise)."""
    if not _is_seq(seq) or len(seq) != n or not all(_is_int(v) for v in seq):
        raise ValueError(f"{who}: {name} must hold one int per {per}, {n} of them")
    return [int(v) for v in seq]


def _size_pair(who: str, what: str, pair) -> Tuple[int, int]:
    """One (h, w): two ints in [1, SIZED_MAX_SIDE], no bools -> the pair as ints (ValueError otherwise, naming it `what`)."""
    if not _is_seq(pair) or len(pair) != 2:
        raise ValueError(f"{who}: {what} must be an (h, w) pair, got {pair!r}")
    h, w = pair
    if not _is_int(h) or not _is_int(w) or not 1 <= int(h) <= SIZED_MAX_SIDE or not 1 <= int(w) <= SIZED_MAX_SIDE:
        raise ValueError(f"{who}: {what} must be two ints in [1, {SIZED_MAX_SIDE}], got {pair!r}")
    return int(h), int(w)


def _plane_sizes(sizes, who: str, name: str = "sizes", n: Optional[int] = None, of: str = "planes") -> list:
    """(h, w) pairs of ints in [1, 16384], no bools -- 1 .. 65535 of them (`of` says of what), or with n= exactly n -> the pairs as ints
    (ValueError otherwise)."""
    if not _is_seq(sizes) or not hasattr(sizes, "__iter__"):
        raise ValueError(f"{who}: {name} must be a sequence of (h, w) pairs, got {type(sizes).__name__}")
    if n is not None and len(sizes) != n:
        raise ValueError(f"{who}: {name} holds {len(sizes)} pairs for {n} images")
    if n is None and not 1 <= len(sizes) <= 65535:
        raise ValueError(f"{who}: 1 .. 65535 {of}, got {len(sizes)}")
    return [_size_pair(who, f"a size of {name}", pair) for pair in sizes]


def _sized_arg(who: str, name: str, s, *, areas: bool = False, boxes: bool = False, optional: bool = False, empty: bool = False):
    """A SizedMasks argument of a utility: 1 .. 65535 planes on the device, with areas / boxes where the utility reads them; optional:
    None passes; empty: so does one without a plane, wherever it lives (ValueError otherwise) -> s."""
    if s is None and optional:
        return None
    ok = isinstance(s, SizedMasks) and not (areas and s.area is None) and not (boxes and s.box is None)
    if ok and not (empty and len(s.sizes) == 0):
        ok = bool(s.bits.is_cuda) and 1 <= len(s.sizes) <= 65535
    if not ok:
        needs = "".join(f", with {what}" for what, on in (("areas", areas), ("boxes", boxes)) if on)
        raise ValueError(f"{who}: {name} must be a SizedMasks of 1 .. 65535 planes on the device{needs}{', or one without a plane' if empty else ''}"
                         f"{', or None' if optional else ''}, got {type(s).__name__}")
    return s


def _per_plane_ints(who: str, name: str, v, P: int, lo: int, hi: int, none: bool = False) -> np.ndarray:
    """One int in [lo, hi] for all P planes or one per plane, no bools; none=True: or None, which is 0 everywhere -> int32 (P,)."""
    if v is None and none:
        return np.zeros(P, dtype=np.int32)
    seq = [v] * P if _is_int(v) else v
    if not _is_seq(seq) or len(seq) != P or not all(_is_int(x) for x in seq):
        raise ValueError(f"{who}: {name} must be {'None, ' if none else ''}an int or hold one int per plane, {P} of them, got {v!r}")
    if not all(lo <= int(x) <= hi for x in seq):
        raise ValueError(f"{who}: {name} must lie in [{lo}, {hi}], got {v!r}")
    return np.asarray([int(x) for x in seq], dtype=np.int32).reshape(P)


def _plane_by_plane(who: str, Pa: int, Pb: int, instead: str = "pairs=") -> np.ndarray:
    """The pairs of a call that names none: plane p of a against plane p of b -> int64 (P, 2)."""
    if Pa != Pb:
        raise ValueError(f"{who}: without {instead} both sides need as many planes, got {Pa} and {Pb}")
    return np.stack([np.arange(Pa)] * 2, axis=1)


def _capped(total: int, one: int, cap: int) -> int:
    """The bytes of a grow-only workspace: what all planes want in flight, up to `cap`, and never below one plane's."""
    return min(total, max(cap, one))


def _upload(a, dev) -> torch.Tensor:
    """One host-to-device copy of a numpy array."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _empty(dev, *shape, dtype=torch.int32) -> torch.Tensor:
    """The allocation of a call's results: an unwritten tensor on dev, int32 unless told; `partial(_empty, dev)` where a call makes many."""
    return torch.empty(*shape, dtype=dtype, device=dev)


def _aligned(t: torch.Tensor) -> torch.Tensor:
    """Detached, contiguous and, where the view starts off a 4-byte boundary, copied: the kernels read packed planes as 32-bit words."""
    t = t.detach().contiguous()
    return t.clone() if t.data_ptr() % 4 != 0 else t


def _integer_map(who: str, name: str, m, int32: bool = True) -> torch.Tensor:
    """A non-empty integer tensor or array as a tensor (ValueError otherwise); int32=True: a host map of a wider type is also held to
    the int32 range, which the kernels read -- a device tensor is the caller's contract, a check would synchronise."""
    t = torch.as_tensor(m) if isinstance(m, (torch.Tensor, np.ndarray)) else None
    if t is None or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool or t.numel() < 1:
        raise ValueError(f"{who}: {name} must be a non-empty integer tensor or array, got {type(m).__name__}")
    if int32 and not t.is_cuda and t.dtype not in (torch.int32, torch.uint8, torch.int16, torch.int8) and \
            (int(t.min()) < -2 ** 31 or int(t.max()) >= 2 ** 31):
        raise ValueError(f"{who}: {name} holds a value outside the int32 range")
    return t


MASK_MODES = ("logits", "bits", "both")
OVERLAP_MAXK = 1024        # hypotheses per image cvlm_mask_overlap takes
OVERLAP_MAXP = 65535       # planes in all it takes


def compact_request(*, masks="logits", overlaps=False, n: int, K: int, who: str = "decode"):
    """Every check of the masks= / overlaps= arguments of Cascade.infer_classes / decode, on the host, before anything
    is launched (ValueError) -> (want_logits, want_bits, want_inter).  n images with K hypotheses each."""
    if not isinstance(masks, str) or masks not in MASK_MODES:
        raise ValueError(f"{who}: masks must be one of {MASK_MODES}, got {masks!r}")
    if not isinstance(overlaps, (bool, np.bool_)):
        raise ValueError(f"{who}: overlaps must be a bool, got {type(overlaps).__name__}")
    if overlaps and masks == "logits":
        raise ValueError(f"{who}: overlaps=True counts packed masks: ask for masks='bits' or 'both'")
    if overlaps and K > OVERLAP_MAXK:
        raise ValueError(f"{who}: overlaps=True takes at most {OVERLAP_MAXK} hypotheses per image (cvlm_mask_overlap), got K = {K}")
    if overlaps and n * K > OVERLAP_MAXP:
        raise ValueError(f"{who}: overlaps=True takes at most {OVERLAP_MAXP} hypotheses in all (cvlm_mask_overlap), got {n} x {K}")
    return masks != "bits", masks != "logits", bool(overlaps)


COMPONENTS_MAXM = 64              # rows of the table cvlm_mask_components selects
COMPONENTS_WS_CAP = 256 << 20     # bytes of the "cls_comp" workspace at most; beyond it the entry walks the planes in rounds


def components_request(*, components=None, min_area=0, connectivity=8, masks="bits", side: Optional[int] = None, who: str = "decode"):
    """Every check of the components= / min_area= / connectivity= arguments of Cascade.infer_classes / decode / mask_components
    (DESIGN.md §14), on the host, before anything is launched (ValueError) -> (asked for, M, min_area, connectivity).  components=None
    with min_area=0 asks for nothing; components=0 asks for the counts without a table.  side: the width of the model's masks."""
    M = 0 if components is None else _int_in(who, "components", components, 0, COMPONENTS_MAXM, none=True)
    min_area, connectivity = _int_in(who, "min_area", min_area, 0), _connectivity(who, connectivity)
    asked = components is not None or min_area > 0
    if asked and masks == "logits":
        raise ValueError(f"{who}: components= / min_area= label packed masks: ask for masks='bits' or 'both'")
    if asked and side is not None and side % 32 != 0:
        raise ValueError(f"{who}: components= / min_area= need rows of whole 32-pixel words, the masks are {side} wide")
    return asked, M, min_area, connectivity


@dataclass
class MaskComponents:
    """Connected regions of N packed masks (Cascade.mask_components); every tensor int32 on the device but kept_bits."""
    n_comp: torch.Tensor                    # (N,) regions per mask
    comps: Optional[torch.Tensor]           # (N, M, 6) the M largest as (area, x0, y0, x1, y1, seed), descending; None with components=0
    n_kept: Optional[torch.Tensor]          # min_area >= 1: (N,) regions of at least min_area pixels, otherwise None like the next three
    kept_bits: Optional[torch.Tensor]       # (N, H * W / 8) uint8 the mask without the smaller regions
    kept_area: Optional[torch.Tensor]       # (N,)
    kept_box: Optional[torch.Tensor]        # (N, 4) inclusive (x0, y0, x1, y1), -1 for an empty result


HOLES_MAXM = 64                   # rows of the table cvlm_mask_holes selects
HOLE_FIELDS = ("n_holes", "holes", "n_filled", "filled_bits", "filled_area")


def holes_request(*, holes=None, fill_holes=0, connectivity=8, masks="bits", side: Optional[int] = None, who: str = "decode"):
    """Every check of the holes= / fill_holes= arguments of Cascade.infer_classes / decode / mask_holes, on the host,
    before anything is launched (ValueError) -> (asked for, M, fill_below, connectivity).  holes=None with fill_holes=0 asks for nothing;
    holes=0 asks for the counts without a table.  connectivity is the foreground's, shared with components=.  side: the width of the
    model's masks."""
    M = 0 if holes is None else _int_in(who, "holes", holes, 0, HOLES_MAXM, none=True)
    fill_holes, connectivity = _int_in(who, "fill_holes", fill_holes, 0, 2 ** 31 - 1), _connectivity(who, connectivity)
    asked = holes is not None or fill_holes > 0
    if asked and masks == "logits":
        raise ValueError(f"{who}: holes= / fill_holes= label packed masks: ask for masks='bits' or 'both'")
    if asked and side is not None and side % 32 != 0:
        raise ValueError(f"{who}: holes= / fill_holes= need rows of whole 32-pixel words, the masks are {side} wide")
    return asked, M, fill_holes, connectivity


@dataclass
class MaskHoles:
    """Holes of N packed masks (Cascade.mask_holes); every tensor int32 on the device but filled_bits."""
    n_holes: torch.Tensor                   # (N,) holes per mask
    holes: Optional[torch.Tensor]           # (N, M, 6) the M largest as (area, x0, y0, x1, y1, seed), descending; None with holes=0
    n_filled: Optional[torch.Tensor]        # fill_holes >= 1: (N,) holes of fewer than fill_holes pixels, otherwise None like the next two
    filled_bits: Optional[torch.Tensor]     # (N, H * W / 8) uint8 the mask with exactly those holes set
    filled_area: Optional[torch.Tensor]     # (N,)


MORPH_MAXR = 16                   # the largest radius cvlm_mask_morph takes
BAND_FIELDS = ("band_bits", "band_area", "band_inter")


def morph_request(*, band=None, masks="bits", overlaps=False, side: Optional[int] = None, who: str = "decode"):
    """Every check of the band= argument of Cascade.infer_classes / decode, on the host, before anything is launched
    (ValueError) -> (asked for, radius, band_inter wanted).  band=None asks for nothing; band=r asks for the edge band by the
    (2 r + 1)^2 square, and with overlaps=True for the bands' pairwise intersections as well.  side: the width of the model's masks."""
    if band is None:
        return False, 0, False
    band = _int_in(who, "band", band, 1, MORPH_MAXR, none=True)
    if masks == "logits":
        raise ValueError(f"{who}: band= is derived from packed masks: ask for masks='bits' or 'both'")
    if side is not None and side % 32 != 0:
        raise ValueError(f"{who}: band= needs rows of whole 32-pixel words, the masks are {side} wide")
    return True, band, bool(overlaps)


@dataclass
class MaskMorph:
    """Dilation, erosion and edge band of N packed masks (Cascade.mask_morph): planes uint8 (N, H * W / 8), areas int32
    (N,), on the device; a pair that was not asked for is None."""
    dil_bits: Optional[torch.Tensor]
    dil_area: Optional[torch.Tensor]
    ero_bits: Optional[torch.Tensor]
    ero_area: Optional[torch.Tensor]
    band_bits: Optional[torch.Tensor]
    band_area: Optional[torch.Tensor]


EDGE_FIELDS = ("edge_bits", "edge_area", "edge_band", "edge_inter")


def _edge_threshold(edge_threshold, who: str) -> float:
    """The threshold as the float32 the kernel compares against, or ValueError: a real number (no bool, no NaN) strictly between 0
    and 1 whose float32 rounding is strictly between 0 and 1 as well."""
    if not _is_real(edge_threshold):
        raise ValueError(f"{who}: edge_threshold must be a real number strictly between 0 and 1, got {edge_threshold!r}")
    t = float(edge_threshold)
    with np.errstate(over="ignore", under="ignore"):
        t32 = float(np.float32(t))
    if not (0.0 < t < 1.0 and 0.0 < t32 < 1.0):                      # NaN fails every comparison
        raise ValueError(f"{who}: edge_threshold must lie strictly between 0 and 1, in float32 as well, got {edge_threshold!r}")
    return t32


def edge_request(*, edge_threshold=None, masks="bits", overlaps=False, band=None, side: Optional[int] = None, who: str = "decode"):
    """Every check of the edge_threshold= argument of Cascade.infer_classes / decode, on the host, before anything is
    launched (ValueError) -> (asked for, the threshold as float32's value, edge_band wanted, edge_inter wanted).  None asks for
    nothing.  The packed edge map sits beside packed masks -- masks="bits" or "both" --; with band= the call also counts the edge
    pixels on each mask's band, with overlaps=True the pairwise intersections of the edge maps.  side: the width of the model's masks."""
    if edge_threshold is None:
        return False, 0.0, False, False
    t = _edge_threshold(edge_threshold, who)
    if masks == "logits":
        raise ValueError(f"{who}: edge_threshold= packs the edge map beside packed masks: ask for masks='bits' or 'both'")
    if side is not None and side % 32 != 0:
        raise ValueError(f"{who}: edge_threshold= needs rows of whole 32-pixel words, the masks are {side} wide")
    return True, t, band is not None, bool(overlaps)


@dataclass
class EdgeBits:
    """N packed edge maps (Cascade.pack_edges), on the device."""
    bits: torch.Tensor              # (N, H * W / 8) uint8, numpy.packbits' order
    area: torch.Tensor              # (N,) int32 set bits
    inter: Optional[torch.Tensor]   # (N,) int32 |bits AND with_bits|; None without with_bits


RLE_WS_CAP = 64 << 20             # bytes of the "cls_rle" workspace at most; beyond it cvlm_mask_rle_emit walks the planes in rounds
RLE_SOURCES = {"mask": "mask_bits", "kept": "kept_bits", "filled": "filled_bits"}
RLE_SIZED = "sized"               # rle="sized": the planes of `sized` (sizes=), each at its image's own size
SIZED_MAX_SIDE = 16384            # h and w of a sized plane (csrc/sized_logic.h: SZ_MAX_SIDE)


def rle_request(*, rle=None, masks="bits", min_area=0, fill_holes=0, side: Optional[int] = None, who: str = "decode"):
    """Every check of the rle= argument of Cascade.infer_classes / decode, on the host, before anything is launched
    (ValueError) -> the name of the field to encode, or None.  rle=None asks for nothing; "mask", "kept" and "filled" ask for the COCO
    run-length encoding of mask_bits, kept_bits (needs min_area >= 1) or filled_bits (needs fill_holes >= 1).  side: the width of the
    model's masks."""
    if rle is None:
        return None
    if isinstance(rle, str) and rle == RLE_SIZED:                    # the sized planes: `sized_request` holds it against sizes=
        if masks == "logits":
            raise ValueError(f"{who}: rle= encodes packed masks: ask for masks='bits' or 'both'")
        return RLE_SIZED
    if not isinstance(rle, str) or rle not in RLE_SOURCES:
        raise ValueError(f"{who}: rle must be None or one of {tuple(RLE_SOURCES) + (RLE_SIZED,)}, got {rle!r}")
    if masks == "logits":
        raise ValueError(f"{who}: rle= encodes packed masks: ask for masks='bits' or 'both'")
    if rle == "kept" and not (_is_int(min_area) and int(min_area) >= 1):
        raise ValueError(f"{who}: rle='kept' encodes kept_bits: ask for min_area >= 1")
    if rle == "filled" and not (_is_int(fill_holes) and int(fill_holes) >= 1):
        raise ValueError(f"{who}: rle='filled' encodes filled_bits: ask for fill_holes >= 1")
    if side is not None and side % 32 != 0:
        raise ValueError(f"{who}: rle= needs rows of whole 32-pixel words, the masks are {side} wide")
    return RLE_SOURCES[rle]


@dataclass
class MaskRle:
    """COCO run-length encoding of N packed masks (Cascade.mask_rle), on the device: plane p's n_runs[p] counts are
    counts[offsets[p] : offsets[p + 1]] -- the lengths of the alternating runs of 0s and 1s of its pixels in column-major order,
    starting with the 0s.  An interchange format, not a compression: a ragged mask has more bytes of counts than of bits."""
    counts: torch.Tensor            # (total,) int32
    offsets: torch.Tensor           # (N + 1,) int64, offsets[0] = 0, offsets[N] = total
    n_runs: torch.Tensor            # (N,) int32
    size: Tuple[int, int]           # (H, W)
    # (1,) int32 on the device, 0 unless cvlm_mask_rle_emit had to drop a count; `check` and `to_coco` read it.  Init-only, not a field.
    status: InitVar[Optional[torch.Tensor]] = None
    # per-plane (h, w) on the host where the planes differ in size (Cascade.mask_rle_sized), otherwise None and every
    # plane is `size`; `to_coco` writes each plane's own.  Init-only, not a field; `size` is then None unless all planes agree.
    sizes: InitVar[Optional[Sequence[Tuple[int, int]]]] = None

    def __post_init__(self, status, sizes):
        self.status = status
        self.sizes = None if sizes is None else [(int(h), int(w)) for h, w in sizes]

    def size_of(self, p: int) -> Tuple[int, int]:
        """(H, W) of plane p."""
        return self.sizes[p] if self.sizes is not None else self.size

    def check(self) -> None:
        """RuntimeError if the emit dropped a count (synchronises).  The slices come from the call's own count of the same bits, so
        this says that the bits changed between the two passes or that the library is broken."""
        if self.status is not None and int(self.status.item()) != 0:
            raise RuntimeError("mask_rle: cvlm_mask_rle_emit dropped counts that did not fit their slices: were the bits written "
                               "while the call ran?")

    def to_coco(self, compressed: bool = False) -> list:
        """On the host: one {"size": [H, W], "counts": ...} per plane (each plane's own size where they differ), what pycocotools and
        the reference's GenericMask (models/utils/visualizer.py:72-101) take; counts is a list of ints, or with compressed=True COCO's
        string as bytes (rle.counts_to_string).  One copy of each of the three tensors; synchronises."""
        from . import rle as _rle
        self.check()
        counts, offsets = self.counts.cpu().numpy(), self.offsets.cpu().numpy()
        out = []
        for p in range(offsets.size - 1):
            H, W = self.size_of(p)
            c = counts[offsets[p]:offsets[p + 1]]
            out.append({"size": [int(H), int(W)], "counts": _rle.counts_to_string(c) if compressed else c.tolist()})
        return out


def sized_tables(plane_sizes):
    """Host tables of sized planes for a list of per-plane (h, w): dims int32 (P, 2), byte offsets int64 (P + 1) --
    plane p is h rows of ceil(w / 32) 32-bit words, the planes lie back to back -- and the largest plane's word count."""
    dims = np.asarray(plane_sizes, dtype=np.int32).reshape(-1, 2)
    words = dims[:, 0].astype(np.int64) * ((dims[:, 1].astype(np.int64) + 31) // 32)
    offsets = np.zeros(dims.shape[0] + 1, dtype=np.int64)
    np.cumsum(4 * words, out=offsets[1:])
    return dims, offsets, int(words.max())


def sized_request(*, sizes=None, sized_level=128, n: int, masks="bits", rle=None, who: str = "decode"):
    """Every check of the sizes= / sized_level= arguments of Cascade.infer_classes / decode and of Cascade.pack_masks_sized (DESIGN.md
    §19), on the host, before anything is launched (ValueError) -> None when nothing is asked for, otherwise (the n (h, w) pairs as
    ints, the level).  sizes: one (h, w) per image of the call, 1 <= h, w <= 16384; sized_level: an int in 1 .. 255, the level the
    reference's uint8 mask is compared with (128: the half; 1: demo.py's `> 0` overlay).  They need packed masks (masks="bits" or
    "both"), and rle="sized" needs sizes=."""
    sized_level = _int_in(who, "sized_level", sized_level, 1, 255)
    if sizes is None:
        if isinstance(rle, str) and rle == RLE_SIZED:
            raise ValueError(f"{who}: rle='sized' encodes the sized planes: give sizes=")
        return None
    if masks == "logits":
        raise ValueError(f"{who}: sizes= packs masks at the images' sizes: ask for masks='bits' or 'both'")
    return _plane_sizes(sizes, who, n=n), sized_level


@dataclass
class SizedMasks:
    """Packed masks at each image's own size (Cascade.pack_masks_sized, sizes= of infer_classes / decode).  Plane p has
    the size sizes[p] = (h, w) and is h rows of ws = ceil(w / 32) 32-bit words in numpy.packbits' order -- the bit order of `mask_bits`
    -- from byte offsets[p] of the flat tensor `bits` on; the pad bits of a row, columns w .. 32 ws - 1, are 0, so that
    `mask_components(plane rows, h, 32 * ws)` and its kin run on one image's planes as they are.  A bit is the reference's uint8 mask
    -- sigmoid, cv2.resize(INTER_LINEAR) to (h, w), (. * 255).astype(uint8) -- compared `>= level`.  At the model's own size these are
    NOT `mask_bits` (logit > 0): they go through the resize's arithmetic with weights 1 and 0 and compare a probability with level / 255."""
    bits: torch.Tensor              # (total bytes,) uint8 on the device
    offsets: torch.Tensor           # (P + 1,) int64 on the device, in bytes, multiples of 4; offsets[P] = bits.numel()
    area: Optional[torch.Tensor]    # (P,) int32 set bits; None from rle_decode(stats=False), like box
    box: Optional[torch.Tensor]     # (P, 4) int32 inclusive (x0, y0, x1, y1) in the image's own coordinates, -1 for an empty plane
    status: torch.Tensor            # int32 on the device, one word per cvlm_mask_pack_sized call: non-zero if a plane was refused
    sizes: list                     # P (h, w) pairs, on the host
    level: int = 128                # 0: not a threshold -- the planes were decoded from run counts (Cascade.rle_decode)
    #                                 or rasterised from polygons (Cascade.polygons_decode, §21)

    @classmethod
    def empty(cls, sizes, dev, *, level: int, stats: bool = True, n_status: int = 1):
        """Unwritten planes of these sizes on `dev`, back to back under offsets of their own (one upload): the bits, area and box (None
        without stats) and n_status status words -> (the SizedMasks, the planes' dims on the host for the caller to upload, the largest
        plane's word count)."""
        dims, offsets, max_words = sized_tables(sizes)
        P, i32 = len(sizes), partial(_empty, dev)
        out = cls(bits=_empty(dev, int(offsets[P]), dtype=torch.uint8), offsets=_upload(offsets, dev), area=i32(P) if stats else None,
                  box=i32(P, 4) if stats else None, status=i32(n_status), sizes=[(int(h), int(w)) for h, w in sizes], level=level)
        return out, dims, max_words

    def tables(self):
        """`sized_tables` of these planes, from `sizes` as they are now: (dims, byte offsets, largest word count) on the host."""
        return sized_tables(self.sizes)

    def byte_range(self, p: int) -> Tuple[int, int]:
        """Where plane p lies in `bits`, from the sizes alone (the planes lie back to back): no read of the device."""
        _, offsets, _ = self.tables()
        return int(offsets[p]), int(offsets[p + 1])

    def plane(self, p: int) -> torch.Tensor:
        """Plane p as a uint8 view (h, 4 * ws) of `bits`: rows in numpy.packbits' order."""
        h, w = self.sizes[p]
        lo, hi = self.byte_range(p)
        return self.bits[lo:hi].view(h, 4 * ((w + 31) // 32))

    def to_numpy(self, p: int) -> np.ndarray:
        """Plane p as a bool array (h, w) on the host (synchronises)."""
        h, w = self.sizes[p]
        return np.unpackbits(self.plane(p).cpu().numpy(), axis=1)[:, :w].astype(bool)

    def check(self) -> None:
        """RuntimeError if the kernel refused a plane (synchronises).  The tables come from the same sizes as the allocation, so this
        says that the library is broken."""
        if bool(self.status.ne(0).any().item()):
            if self.level == 0:
                raise RuntimeError("rle_decode / polygons_decode: cvlm_mask_rle_decode or cvlm_mask_poly_decode refused a plane: counts that "
                                   "are negative or do not sum to h * w, a polygon outside the bounds, or a slice that does not fit")
            raise RuntimeError("pack_masks_sized: cvlm_mask_pack_sized refused a plane whose slice did not fit its size")

    @staticmethod
    def concat(parts) -> "SizedMasks":
        """The planes of several SizedMasks of one device as one, in the order of `parts`, on the device and without a synchronisation:
        `torch.cat` of bits, areas and boxes, each part's offsets shifted by the bytes before it, the sizes appended, the status words
        ORed into one.  What it is for: `polygons_decode` of an image set's iscrowd = 0 annotations and `rle_decode` of its crowd regions
        as ONE ground_truth= -- the image ids given with it carry the association, so the order is free.  Parts with
        and without area / box do not mix (ValueError); the level is kept where all parts share it and is 0 otherwise."""
        if isinstance(parts, SizedMasks) or not _is_seq(parts) or len(parts) < 1 or not all(isinstance(s, SizedMasks) for s in parts):
            raise ValueError("SizedMasks.concat: a non-empty sequence of SizedMasks")
        parts = list(parts)
        if len({s.area is None for s in parts}) != 1 or any((s.area is None) != (s.box is None) for s in parts):
            raise ValueError("SizedMasks.concat: parts with and without area / box do not mix")
        if len({s.bits.device for s in parts}) != 1:
            raise ValueError("SizedMasks.concat: the parts live on different devices")
        sizes = [tuple(z) for s in parts for z in s.sizes]
        starts = np.cumsum([0] + [s.tables()[1][-1] for s in parts[:-1]])                 # from the sizes alone: no read of the device
        offsets = torch.cat([parts[0].offsets] + [s.offsets[1:] + int(b) for s, b in zip(parts[1:], starts[1:])])
        stats = parts[0].area is not None
        status = parts[0].status.reshape(-1).ne(0).any().to(torch.int32).reshape(1)
        for s in parts[1:]:
            status = status | s.status.reshape(-1).ne(0).any().to(torch.int32).reshape(1)
        levels = {s.level for s in parts}
        return SizedMasks(bits=torch.cat([s.bits for s in parts]), offsets=offsets,
                          area=torch.cat([s.area for s in parts]) if stats else None,
                          box=torch.cat([s.box for s in parts]) if stats else None, status=status, sizes=sizes,
                          level=levels.pop() if len(levels) == 1 else 0)


LABELS_MAX_K = 16384              # hypotheses per image of a label map: a winner is an int16 (csrc/labels_logic.h: LB_MAX_K)
LABELS_MAX_CLASSES = 65536        # classes of Cascade.label_iou (LB_MAX_C)


def label_tables(sizes):
    """Host tables of label maps for a list of per-image (h, w): dims int32 (B, 2), pixel offsets int64 (B + 1) -- image
    b's map is its h * w entries, row pitch w, the images lie back to back -- and the largest image's pixel count."""
    dims = np.asarray(sizes, dtype=np.int32).reshape(-1, 2)
    pixels = dims[:, 0].astype(np.int64) * dims[:, 1].astype(np.int64)
    offsets = np.zeros(dims.shape[0] + 1, dtype=np.int64)
    np.cumsum(pixels, out=offsets[1:])
    return dims, offsets, int(pixels.max())


def labels_request(*, label_maps=False, sizes=None, weights=None, level=128, overlap_threshold=0.8, n: int, K: int, masks="bits",
                   who: str = "decode"):
    """Every check of the label_maps= / label_weights= / overlap_threshold= arguments of Cascade.infer_classes / decode and of
    Cascade.label_maps, on the host, before anything is launched (ValueError) -> None when no label maps are asked
    for, otherwise (weights, level, overlap_threshold): weights is None (every weight 1), a float32 numpy array (n * K,) to upload, or
    the caller's device tensor.  Label maps live at the images' own sizes: they need sizes= (checked by `sized_request`) and packed
    masks; K <= 16384; level an int in 1 .. 255; overlap_threshold a real in (0, 1]; weights one f32 per hypothesis -- a host
    sequence of n * K reals or n rows of K, none of them NaN, or a float32 device tensor of shape (n, K) or (n * K,)."""
    if not isinstance(label_maps, (bool, np.bool_)):
        raise ValueError(f"{who}: label_maps must be a bool, got {label_maps!r}")
    if not label_maps:
        if weights is not None:
            raise ValueError(f"{who}: label_weights= weighs the hypotheses of a label map: ask for label_maps=True")
        return None
    if sizes is None:
        raise ValueError(f"{who}: label maps live at the images' own sizes: give sizes=")
    if masks == "logits":
        raise ValueError(f"{who}: label_maps=True goes with the packed masks: ask for masks='bits' or 'both'")
    if not 1 <= K <= LABELS_MAX_K:
        raise ValueError(f"{who}: a label map holds 1 .. {LABELS_MAX_K} hypotheses per image, got K = {K}")
    level = _int_in(who, "the level of a label map", level, 1, 255)
    if not _is_real(overlap_threshold) or not 0.0 < float(overlap_threshold) <= 1.0:      # a NaN fails the comparison too
        raise ValueError(f"{who}: overlap_threshold must be a real in (0, 1], got {overlap_threshold!r}")
    if isinstance(weights, torch.Tensor) and weights.is_cuda:
        if weights.dtype != torch.float32 or tuple(weights.shape) not in ((n, K), (n * K,)):
            raise ValueError(f"{who}: label weights on the device must be float32 of shape ({n}, {K}), got {weights.dtype} "
                             f"{tuple(weights.shape)}")
    elif weights is not None:
        try:
            host = np.asarray(weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else weights, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: label weights must be reals, one per hypothesis") from None
        if host.shape not in ((n, K), (n * K,)):
            raise ValueError(f"{who}: label weights hold {host.shape} entries for {n} images of {K} hypotheses")
        if np.isnan(host).any():
            raise ValueError(f"{who}: a label weight is NaN: leave the hypothesis out with class -1 instead")
        weights = np.ascontiguousarray(host.reshape(-1), dtype=np.float32)
    return weights, level, float(overlap_threshold)


@dataclass
class LabelMaps:
    """One hypothesis per pixel at each image's own size (Cascade.label_maps, label_maps=True of infer_classes / decode; DESIGN.md
    §23): Mask2Former's panoptic_inference over the K hypotheses of each image.  Image b's maps are its h * w entries, row pitch w,
    from entry pix_offsets[b] of the flat tensors on.  All tensors on the device; nothing here synchronises but `check` and `to_host`."""
    score: torch.Tensor             # (pixels,) f32: the winner's s = weight * value
    winner: torch.Tensor            # (pixels,) int16: the k with the largest s (ties: the smallest k), -1 where no hypothesis takes part
    segment: torch.Tensor           # (pixels,) int16: k where winner = k, k's own sized bit is set and k is kept; else -1
    areas: torch.Tensor             # (3, B * K) int32: orig_area (|bit_k|), won_area (|winner = k|), kept_area (|winner = k and bit_k|)
    segment_id: torch.Tensor        # (B * K,) int32: 1, 2, ... over the kept hypotheses of an image in increasing k; 0 = not kept
    n_segments: torch.Tensor        # (B,) int32
    status: torch.Tensor            # (1,) int32: non-zero if a kernel refused an image
    dims: torch.Tensor              # (B, 2) int32 (h, w)
    pix_offsets: torch.Tensor       # (B + 1,) int64, in pixels
    sizes: list                     # B (h, w) pairs, on the host
    K: int
    level: int = 128
    overlap_threshold: float = 0.8

    @property
    def B(self) -> int:
        return len(self.sizes)

    @property
    def kept(self) -> torch.Tensor:
        """(B, K) bool: the hypotheses that own a segment."""
        return self.segment_id.view(self.B, self.K) > 0

    def _range(self, b: int) -> Tuple[int, int]:
        _, offsets, _ = label_tables(self.sizes)                      # from the sizes alone: no read of the device
        return int(offsets[b]), int(offsets[b + 1])

    def image_of(self, flat: torch.Tensor, b: int) -> torch.Tensor:
        """Image b's (h, w) view of a flat per-pixel tensor of these maps -- `winner`, `segment`, or what `categories` returned."""
        lo, hi = self._range(b)
        return flat[lo:hi].view(*self.sizes[b])

    def winner_of(self, b: int) -> torch.Tensor:
        return self.image_of(self.winner, b)

    def segment_of(self, b: int) -> torch.Tensor:
        return self.image_of(self.segment, b)

    def check(self) -> None:
        """RuntimeError if a kernel refused an image (synchronises).  The tables come from the same sizes as the allocation, so this
        says that the library is broken."""
        if bool(self.status.ne(0).any().item()):
            raise RuntimeError("label_maps: a cvlm_label_* kernel refused an image whose slice did not fit its size")

    def _lookup(self, table: torch.Tensor, which: str, void: int) -> torch.Tensor:
        if which not in ("winner", "segment"):
            raise ValueError(f"LabelMaps: which must be 'winner' or 'segment', got {which!r}")
        void = _int_in("LabelMaps", "void", void, -2 ** 31, 2 ** 31 - 1)
        out = torch.empty(self.winner.numel(), dtype=torch.int32, device=self.winner.device)
        _, _, max_pixels = label_tables(self.sizes)
        hip.label_lookup(getattr(self, which), self.B, self.K, self.dims, self.pix_offsets, max_pixels, table, void, out, self.status)
        return out

    def categories(self, labels, which: str = "winner", void: int = 255) -> torch.Tensor:
        """The maps as class maps: (pixels,) int32 = labels[b, k] where the map holds k, `void` where it holds -1 (cvlm_label_lookup).
        labels: (B, K) integers, e.g. `classes` of the call -- which="winner": the semantic map (MaskFormer's semantic inference with
        one class per query); which="segment": the panoptic category map.  `image_of(result, b)` is image b's (h, w) view."""
        t = torch.as_tensor(labels)
        if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool or tuple(t.shape) not in ((self.B, self.K), (self.B * self.K,)):
            raise ValueError(f"LabelMaps.categories: labels must be ({self.B}, {self.K}) integers, got {t.dtype} {tuple(t.shape)}")
        table = t.to(device=self.winner.device, dtype=torch.int32).contiguous().view(-1)
        return self._lookup(table, which, void)

    def panoptic(self) -> torch.Tensor:
        """The published `panoptic_seg`: (pixels,) int32 segment ids 1 .. n_segments[b], 0 where no segment holds the pixel."""
        return self._lookup(self.segment_id, "segment", 0)

    def pq_inputs(self, labels) -> Tuple[torch.Tensor, torch.Tensor]:
        """The panoptic map in the form Cascade.panoptic_quality scores -> (pred, pred_cat), no synchronisation: pred
        (pixels,) int32 = k + 1 where `segment` holds k, 0 (void) elsewhere (cvlm_label_lookup); pred_cat (B, K + 1) int32 on the device
        = labels[b, k] in slot k + 1, -1 in slot 0.  labels: (B, K) integers, e.g. `classes` of the call.  So S = K + 1; a hypothesis
        that was not kept owns no pixel, and a slot without a pixel is skipped by the matching."""
        t = torch.as_tensor(labels)
        if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool or tuple(t.shape) not in ((self.B, self.K), (self.B * self.K,)):
            raise ValueError(f"LabelMaps.pq_inputs: labels must be ({self.B}, {self.K}) integers, got {t.dtype} {tuple(t.shape)}")
        dev = self.winner.device
        slots = torch.arange(1, self.K + 1, dtype=torch.int32, device=dev).repeat(self.B)
        pred_cat = torch.full((self.B, self.K + 1), -1, dtype=torch.int32, device=dev)
        pred_cat[:, 1:] = t.to(device=dev, dtype=torch.int32).view(self.B, self.K)
        return self._lookup(slots, "segment", 0), pred_cat

    def to_host(self) -> dict:
        """Everything as numpy arrays in one read-back (synchronises): winner / segment as lists of (h, w) int16 arrays, orig_area /
        won_area / kept_area / segment_id (B, K) int32, kept (B, K) bool, n_segments (B,), status."""
        self.check()
        B, K = self.B, self.K
        winner, segment = self.winner.cpu().numpy(), self.segment.cpu().numpy()
        areas = self.areas.cpu().numpy().reshape(3, B, K)
        ids = self.segment_id.cpu().numpy().reshape(B, K)
        cut = lambda flat: [flat[slice(*self._range(b))].reshape(self.sizes[b]) for b in range(B)]
        return dict(winner=cut(winner), segment=cut(segment), orig_area=areas[0], won_area=areas[1], kept_area=areas[2], segment_id=ids,
                    kept=ids > 0, n_segments=self.n_segments.cpu().numpy(), status=int(self.status.cpu().item()))


PQ_MAX_CELLS = 1 << 24            # G * S of Cascade.panoptic_quality (csrc/panoptic_logic.h: PN_MAX_CELLS)


def _pq_table(who: str, name: str, table, B: int, dtype):
    """One slot table of pq_request: a device tensor is the caller's contract beyond shape and dtype (a look would synchronise); anything
    else becomes a numpy array (B, slots) of `dtype`."""
    if isinstance(table, torch.Tensor) and table.is_cuda:
        want = torch.int32 if dtype is np.int32 else torch.uint8
        if table.dtype != want or table.dim() != 2 or table.shape[0] != B or table.shape[1] < 1:
            raise ValueError(f"{who}: {name} on the device must be {want} of shape ({B}, slots), got {table.dtype} {tuple(table.shape)}")
        return table
    try:
        host = np.asarray(table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else table)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} must be integers of shape ({B}, slots)") from None
    if host.dtype == object or not (np.issubdtype(host.dtype, np.integer) or host.dtype == np.bool_) or host.ndim != 2 \
            or host.shape[0] != B or host.shape[1] < 1:
        raise ValueError(f"{who}: {name} must be integers of shape ({B}, slots), got {host.dtype} {host.shape}")
    if dtype is np.int32 and host.dtype == np.bool_:
        raise ValueError(f"{who}: {name} must be integers, got bool")
    return host


def _image_sizes(sizes, who: str) -> list:
    """The 1 .. 65535 (h, w) at which the maps of a panoptic call lie image by image -> the pairs as ints (ValueError otherwise)."""
    if sizes is None:
        raise ValueError(f"{who}: the maps lie image by image at the images' own sizes: give sizes")
    return _plane_sizes(sizes, who, of="images")


def pq_request(pred_cat, gt_cat, gt_crowd, sizes, *, num_classes, n_pred: int, n_gt: int, who: str = "panoptic_quality"):
    """Every check of the arguments of Cascade.panoptic_quality, on the host, before anything is launched (ValueError)
    -> (the B (h, w) pairs, pred_cat, gt_cat, gt_crowd, G, S): a table is an int32 / uint8 numpy array to upload, or the caller's device
    tensor.  num_classes an int in [1, 65536]; sizes as `sized_request` has them, and n_pred = n_gt = their pixels; pred_cat (B, S)
    and gt_cat (B, G) integers in [-1, num_classes) with -1 in slot 0, which is void; gt_crowd (B, G) of 0 / 1; G * S <= 2^24.  A host
    table is checked value by value; of a device tensor only shape and dtype are (the kernels read a category outside [0,
    num_classes) as "slot unused")."""
    num_classes = _int_in(who, "num_classes", num_classes, 1, LABELS_MAX_CLASSES)
    sizes = _image_sizes(sizes, who)
    B = len(sizes)
    pixels = sum(h * w for h, w in sizes)
    if n_pred != n_gt:
        raise ValueError(f"{who}: pred holds {n_pred} pixels, gt {n_gt}")
    if n_pred != pixels:
        raise ValueError(f"{who}: the maps hold {n_pred} pixels, sizes {pixels}")
    pred_cat = _pq_table(who, "pred_cat", pred_cat, B, np.int32)
    gt_cat = _pq_table(who, "gt_cat", gt_cat, B, np.int32)
    gt_crowd = _pq_table(who, "gt_crowd", gt_crowd, B, np.uint8)
    S, G = int(pred_cat.shape[1]), int(gt_cat.shape[1])
    if tuple(gt_crowd.shape) != (B, G):
        raise ValueError(f"{who}: gt_crowd must have gt_cat's shape ({B}, {G}), got {tuple(gt_crowd.shape)}")
    if G * S > PQ_MAX_CELLS:
        raise ValueError(f"{who}: {G} ground-truth slots x {S} predicted slots: the pair table holds at most 2^24 cells")
    for name, t in (("pred_cat", pred_cat), ("gt_cat", gt_cat)):
        if isinstance(t, torch.Tensor):
            continue
        if int(t.min()) < -1 or int(t.max()) >= num_classes:
            raise ValueError(f"{who}: {name} holds a category outside [-1, {num_classes})")
        if (t[:, 0] != -1).any():
            raise ValueError(f"{who}: slot 0 of {name} is void and must be -1")
    if not isinstance(gt_crowd, torch.Tensor) and gt_crowd.dtype != np.bool_ and (int(gt_crowd.min()) < 0 or int(gt_crowd.max()) > 1):
        raise ValueError(f"{who}: gt_crowd holds a value that is neither 0 nor 1")
    as_np = lambda t, dt: t if isinstance(t, torch.Tensor) else np.ascontiguousarray(t, dtype=dt)
    return sizes, as_np(pred_cat, np.int32), as_np(gt_cat, np.int32), as_np(gt_crowd, np.uint8), G, S


def pq_segments_request(segments, B: int, *, num_classes=None, who: str = "panoptic_remap"):
    """The per-image `segments_info` of Cascade.panoptic_remap -- per image a list of (id, category, iscrowd) in annotation order -- as the
    kernels' tables (ValueError otherwise) -> (keys int32, vals int32, table_offsets int64 (B + 1,), gt_cat int32 (B, G), gt_crowd uint8
    (B, G)): keys ascending per image, vals the 1-based position in the annotation, G = the largest count + 1.  An id is an int in [1,
    2^24) (0 is void), unique within its image; a category an int >= 0 (below num_classes where that is given)."""
    if not _is_seq(segments) or len(segments) != B or not all(hasattr(s, "__len__") for s in segments):
        raise ValueError(f"{who}: segments must hold one list of (id, category, iscrowd) per image, {B} in all")
    G = max([len(s) for s in segments] + [0]) + 1
    keys, vals, offsets = [], [], [0]
    gt_cat, gt_crowd = np.full((B, G), -1, np.int32), np.zeros((B, G), np.uint8)
    for b, segs in enumerate(segments):
        ids = []
        for i, seg in enumerate(segs):
            if not _is_seq(seg) or len(seg) != 3:
                raise ValueError(f"{who}: a segment is (id, category, iscrowd), got {seg!r}")
            sid, cat, crowd = seg
            if not _is_int(sid) or not 1 <= int(sid) < 2 ** 24:
                raise ValueError(f"{who}: a segment id must be an int in [1, 2^24), got {sid!r}")
            if not _is_int(cat) or int(cat) < 0 or (num_classes is not None and int(cat) >= int(num_classes)):
                raise ValueError(f"{who}: a segment's category must be an int >= 0 and below num_classes, got {cat!r}")
            if crowd not in (0, 1, False, True):
                raise ValueError(f"{who}: iscrowd must be 0 or 1, got {crowd!r}")
            ids.append(int(sid))
            gt_cat[b, i + 1], gt_crowd[b, i + 1] = int(cat), int(crowd)
        if len(set(ids)) != len(ids):
            raise ValueError(f"{who}: image {b} lists a segment id twice")
        order = np.argsort(np.asarray(ids, np.int64), kind="stable")
        keys += [ids[i] for i in order]
        vals += [int(i) + 1 for i in order]
        offsets.append(len(keys))
    return (np.asarray(keys or [0], np.int32), np.asarray(vals or [0], np.int32), np.asarray(offsets, np.int64), gt_cat, gt_crowd)


@dataclass
class PanopticGroundTruth:
    """What Cascade.panoptic_remap returns: a ground-truth id map as dense slot indices with the slot tables
    Cascade.panoptic_quality takes.  Tensors on the device; nothing here synchronises but `check`."""
    gt: torch.Tensor                # (pixels,) int32: 1 + the position of the pixel's segment in its image's annotation, 0 = void
    unknown: torch.Tensor           # (B,) int32: pixels whose non-zero raw id the annotation does not list (they became void)
    gt_cat: np.ndarray              # (B, G) int32: category per slot, -1 = unused, slot 0 void
    gt_crowd: np.ndarray            # (B, G) uint8: iscrowd per slot
    status: torch.Tensor            # (1,) int32: non-zero if the kernel refused an image
    sizes: list

    def check(self) -> None:
        if bool(self.status.ne(0).any().item()):
            raise RuntimeError("panoptic_remap: cvlm_pan_remap refused an image whose slice did not fit its size")


@dataclass
class PanopticTotals:
    """What Cascade.panoptic_quality returns: a dataset's sums, into which further calls accumulate (`totals=`), and the
    per-image matching of the last call.  All tensors on the device; nothing here synchronises but `check` and `to_host`."""
    counts: torch.Tensor            # (3, C) int64: tp, fp, fn per category
    iou_sum: torch.Tensor           # (C,) f64: the sum of the true positives' IoU per category
    status: torch.Tensor            # (1,) int32: 1 = a kernel refused an image, 2 = a map held an index outside its slot table
    inter: torch.Tensor             # (B, G, S) int32: the last call's pair counts
    pred_match: torch.Tensor        # (B, S) int32: the matched g, 0 = unused / no pixel / void, -1 = false positive, -2 = ignored
    pred_iou: torch.Tensor          # (B, S) f64
    gt_match: torch.Tensor          # (B, G) int32: the matched s, 0 = unused / void, -1 = false negative, -2 = crowd
    pred_area: torch.Tensor         # (B, S) int32
    gt_area: torch.Tensor           # (B, G) int32
    num_classes: int

    def check(self) -> None:
        """RuntimeError if a kernel refused an image or met an index outside its table, in any call summed so far (synchronises)."""
        s = int(self.status.cpu().item())
        if s & 1:
            raise RuntimeError("panoptic_quality: a cvlm_pan_* kernel refused an image whose slice did not fit its size")
        if s & 2:
            raise RuntimeError("panoptic_quality: a map holds a segment index outside its slot table; such pixels were counted nowhere")

    def to_host(self) -> dict:
        """Everything as numpy arrays in one read-back (synchronises); `segeval.pq_average(counts, iou_sum)` gives PQ, SQ and RQ."""
        self.check()
        names = ("counts", "iou_sum", "inter", "pred_match", "pred_iou", "gt_match", "pred_area", "gt_area")
        return dict({n: getattr(self, n).cpu().numpy() for n in names}, status=0)


def rle_decode_request(rles, who: str = "rle_decode"):
    """Every check of a list of COCO run-length dicts {"size": [h, w], "counts": list | bytes | str}, on the host, before
    anything is launched (ValueError) -> (counts int32 (total,), run offsets int64 (P + 1,) in elements of counts, the P (h, w) pairs).
    A string is COCO's compressed form (rle.string_to_counts).  h and w are ints in [1, 16384]; the counts are non-negative -- zeros are
    legal anywhere, pycocotools emits them -- and sum to h * w."""
    from . import rle as _rle
    if isinstance(rles, dict) or not _is_seq(rles) or not hasattr(rles, "__iter__"):
        raise ValueError(f"{who}: rles must be a sequence of COCO dicts, got {type(rles).__name__}")
    if not 1 <= len(rles) <= 65535:
        raise ValueError(f"{who}: 1 .. 65535 planes, got {len(rles)}")
    sizes, parts = [], []
    for i, d in enumerate(rles):
        if not isinstance(d, dict) or "size" not in d or "counts" not in d:
            raise ValueError(f"{who}: entry {i} must be a dict with 'size' and 'counts'")
        h, w = _size_pair(who, f"entry {i}: size", d["size"])
        c = d["counts"]
        if isinstance(c, (bytes, str)):
            c = _rle.string_to_counts(c)
        else:
            if isinstance(c, dict) or not hasattr(c, "__len__"):
                raise ValueError(f"{who}: entry {i}: counts must be a list of ints, bytes or str, got {type(c).__name__}")
            if not isinstance(c, np.ndarray) and not all(_is_int(v) for v in c):
                raise ValueError(f"{who}: entry {i}: counts must hold ints")
            c = np.asarray(c)
            if c.ndim != 1 or (c.size and c.dtype.kind not in "iu"):
                raise ValueError(f"{who}: entry {i}: counts must be a flat sequence of ints")
            c = c.astype(np.int64)
        if c.size == 0 or bool((c < 0).any()) or int(c.sum()) != h * w:
            raise ValueError(f"{who}: entry {i}: {c.size} counts summing to {int(c.sum())} do not describe a plane of {h} x {w}")
        sizes.append((h, w))
        parts.append(c.astype(np.int32))
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([p.size for p in parts], out=offsets[1:])
    return np.concatenate(parts), offsets, sizes


POLY_MAX_COORD = 65536.0          # |c| of a polygon's coordinates (csrc/poly_logic.h)
POLY_MAX_VERTS = 65535            # vertices of a polygon, 3 at least
POLY_MAX_POINTS = 1 << 24         # walk points of a polygon
POLY_MAX_POLYS = 4096             # polygons of a plane


def polygons_request(anns, who: str = "polygons_decode"):
    """Every check of a list of COCO polygon annotations {"size": [h, w], "polygons": [[x0, y0, x1, y1, ...], ...]} --
    `polygons` is what an iscrowd = 0 annotation's `segmentation` holds --, on the host, before anything is launched (ValueError) ->
    (xy float64 (total,), polygon offsets int64 (Q + 1,) in doubles of xy, plane_polys int32 (P + 1,), the P (h, w) pairs).  1 ..
    65535 planes; h and w ints in [1, 16384]; 1 .. 4096 polygons per plane; a polygon is a flat sequence of an even number of real
    numbers, 3 .. 65535 vertices, finite, |c| <= 65536, and walks at most 2^24 points -- counted here as the kernel counts them, in
    numpy over the polygon's vertices."""
    if isinstance(anns, dict) or not _is_seq(anns) or not hasattr(anns, "__iter__"):
        raise ValueError(f"{who}: anns must be a sequence of dicts with 'size' and 'polygons', got {type(anns).__name__}")
    if not 1 <= len(anns) <= 65535:
        raise ValueError(f"{who}: 1 .. 65535 planes, got {len(anns)}")
    sizes, parts, per_plane = [], [], []
    for i, d in enumerate(anns):
        if not isinstance(d, dict) or "size" not in d or "polygons" not in d:
            raise ValueError(f"{who}: entry {i} must be a dict with 'size' and 'polygons'")
        size = _size_pair(who, f"entry {i}: size", d["size"])
        polys = d["polygons"]
        if isinstance(polys, dict) or not _is_seq(polys) or not 1 <= len(polys) <= POLY_MAX_POLYS:
            raise ValueError(f"{who}: entry {i}: polygons must be a list of 1 .. {POLY_MAX_POLYS} polygons")
        for j, poly in enumerate(polys):
            if isinstance(poly, dict) or not _is_seq(poly):
                raise ValueError(f"{who}: entry {i}, polygon {j}: a flat sequence of numbers, got {type(poly).__name__}")
            try:
                a = np.asarray(poly)
            except Exception as e:
                raise ValueError(f"{who}: entry {i}, polygon {j}: a flat sequence of numbers") from e
            if a.ndim != 1 or a.dtype.kind not in "iuf" or (not isinstance(poly, np.ndarray) and any(isinstance(v, (bool, np.bool_)) for v in poly)):
                raise ValueError(f"{who}: entry {i}, polygon {j}: a flat sequence of real numbers")
            if a.size % 2 or not 6 <= a.size <= 2 * POLY_MAX_VERTS:
                raise ValueError(f"{who}: entry {i}, polygon {j}: {a.size} numbers are no 3 .. {POLY_MAX_VERTS} vertices (x, y)")
            a = a.astype(np.float64)
            if not bool(np.isfinite(a).all()) or float(np.abs(a).max()) > POLY_MAX_COORD:
                raise ValueError(f"{who}: entry {i}, polygon {j}: coordinates must be finite and within +-{POLY_MAX_COORD:.0f}")
            v = (5.0 * a + 0.5).astype(np.int64).reshape(-1, 2)       # csrc/poly_logic.h: pl_scale; astype truncates toward zero
            step = np.abs(np.roll(v, -1, axis=0) - v).max(axis=1) + 1   # pl_edge_of's n, the closing edge included
            if int(step.sum()) > POLY_MAX_POINTS:
                raise ValueError(f"{who}: entry {i}, polygon {j}: {int(step.sum())} walk points, at most {POLY_MAX_POINTS} are taken")
            parts.append(a)
        sizes.append(size)
        per_plane.append(len(polys))
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([p.size for p in parts], out=offsets[1:])
    plane_polys = np.zeros(len(sizes) + 1, dtype=np.int32)
    np.cumsum(per_plane, out=plane_polys[1:])
    return np.concatenate(parts), offsets, plane_polys, sizes


def pairs_request(a_sizes, b_sizes, *, pairs=None, a_image=None, b_image=None, who: str = "mask_inter_sized"):
    """Every check of the pairs of Cascade.mask_inter_sized that the host can make, before anything is launched
    (ValueError) -> int32 (N, 2) on the host, or the caller's device tensor as it is.  Either pairs= -- (N, 2) ints (plane of a, plane of
    b), in range; a tensor on the device is only checked by shape and left to the kernel --, or a_image= and b_image=, one image id per
    plane of each: all (p, q) with a_image[p] == b_image[q], ordered by p, then q.  1 <= N <= 2^20."""
    Pa, Pb = len(a_sizes), len(b_sizes)
    if (pairs is None) == (a_image is None and b_image is None) or (a_image is None) != (b_image is None):
        raise ValueError(f"{who}: give either pairs= or both a_image= and b_image=")
    if pairs is not None:
        if isinstance(pairs, torch.Tensor) and pairs.is_cuda:
            if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype not in (torch.int32, torch.int64) or not 1 <= pairs.shape[0] <= 1 << 20:
                raise ValueError(f"{who}: pairs on the device must be an integer tensor (N, 2), 1 <= N <= 2^20")
            return pairs
        try:
            arr = np.asarray(pairs.cpu() if isinstance(pairs, torch.Tensor) else pairs)
        except Exception as e:
            raise ValueError(f"{who}: pairs must be (N, 2) ints") from e
        if arr.ndim != 2 or arr.shape[1] != 2 or arr.dtype.kind not in "iu" or not 1 <= arr.shape[0] <= 1 << 20:
            raise ValueError(f"{who}: pairs must be (N, 2) ints, 1 <= N <= 2^20")
        if bool((arr < 0).any()) or bool((arr[:, 0] >= Pa).any()) or bool((arr[:, 1] >= Pb).any()):
            raise ValueError(f"{who}: a pair names a plane outside [0, {Pa}) x [0, {Pb})")
        return np.ascontiguousarray(arr.astype(np.int32))
    ids = [np.asarray(_int_list(who, name, seq, P), dtype=np.int64) for name, seq, P in (("a_image", a_image, Pa), ("b_image", b_image, Pb))]
    p, q = np.nonzero(ids[0][:, None] == ids[1][None, :])             # row-major: ordered by p, then q
    if not 1 <= p.size <= 1 << 20:
        raise ValueError(f"{who}: the image ids give {p.size} pairs, 1 .. 2^20 are taken")
    return np.ascontiguousarray(np.stack([p, q], axis=1).astype(np.int32))


MATCH_CAP = 1024                  # detections, and annotations, of one group (csrc/match_logic.h)
MATCH_MAX_T, MATCH_MAX_A = 16, 8
MATCH_IOU_THRS = tuple(np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True).tolist())     # COCO's ten
MATCH_AREA_RNGS = ((0.0, 1e5 ** 2), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e5 ** 2))             # all, small, medium, large


BOUNDARY_MAX_RADIUS = 16384       # the radius of a boundary (csrc/boundary_logic.h: BD_MAX_RADIUS)
BOUNDARY_RATIO = 0.02             # boundary_iou_api's dilation_ratio: the radius is this share of the image's diagonal


def boundary_radius(h: int, w: int, ratio: float = BOUNDARY_RATIO) -> int:
    """The radius of the boundary of an h x w image, exactly as boundary_iou_api's mask_to_boundary forms it: float64,
    Python's round (half to even), at least 1.  (480, 640) -> 16, (1024, 1024) -> 29, (100, 75) -> 2: the product is exactly 2.5."""
    return max(1, int(round(ratio * np.sqrt(h ** 2 + w ** 2))))


def boundary_request(sizes, *, dilation_ratio=BOUNDARY_RATIO, radius=None, who: str = "mask_boundary_sized") -> np.ndarray:
    """Every check of the dilation_ratio= / radius= arguments of Cascade.mask_boundary_sized and of boundary= of Cascade.coco_match
    (DESIGN.md §25), on the host, before anything is launched (ValueError) -> the radius of each plane of `sizes`, int32 (P,).
    dilation_ratio: a finite real > 0 (no bool), the share of each plane's own diagonal (`boundary_radius`); a plane whose radius would
    exceed 16384 is refused.  radius: instead of it, one int in [1, 16384] for all planes or one per plane (no bools); together with a
    dilation_ratio other than the default it is a contradiction."""
    if not _is_real(dilation_ratio) or not np.isfinite(float(dilation_ratio)) or not float(dilation_ratio) > 0.0:
        raise ValueError(f"{who}: the dilation ratio must be a finite real > 0, got {dilation_ratio!r}")
    P = len(sizes)
    if radius is None:
        out = [boundary_radius(int(h), int(w), float(dilation_ratio)) for h, w in sizes]
        if any(d > BOUNDARY_MAX_RADIUS for d in out):
            raise ValueError(f"{who}: a dilation ratio of {dilation_ratio!r} gives a radius above {BOUNDARY_MAX_RADIUS}")
        return np.asarray(out, dtype=np.int32).reshape(P)
    if float(dilation_ratio) != BOUNDARY_RATIO:
        raise ValueError(f"{who}: give either radius= or a dilation ratio, not both")
    return _per_plane_ints(who, "radius", radius, P, 1, BOUNDARY_MAX_RADIUS)


CONTOUR_MAX_VERTS = 1 << 22       # vertices of one plane's contour (csrc/contour_logic.h: CT_MAX_VERTS)


def contour_request(sizes, *, connectivity=8, who: str = "mask_contours_sized"):
    """Every check of the arguments of Cascade.mask_contours_sized, on the host, before anything is launched
    (ValueError) -> (the (h, w) pairs as ints, the connectivity).  sizes: 1 .. 65535 pairs of ints in [1, 16384], no bools;
    connectivity: the int 4 or 8, no bool -- how the foreground hangs together where two pixels touch at a corner."""
    connectivity = _connectivity(who, connectivity)
    return _plane_sizes(sizes, who), connectivity


def contour_rounds(n_vertices, max_words: int, cap: int, need) -> list:
    """The rounds of Cascade.mask_contours_sized: consecutive planes [a, b) taken while need(b - a, their vertices, max_words) stays
    within `cap` bytes, one plane at least -> [(a, b, vertices, bytes)].  Pure host arithmetic; `need` is
    hip.mask_contour_workspace_bytes."""
    out, a, P = [], 0, len(n_vertices)
    while a < P:
        b, rv = a + 1, int(n_vertices[a])
        while b < P and need(b + 1 - a, rv + int(n_vertices[b]), max_words) <= cap:
            rv += int(n_vertices[b])
            b += 1
        out.append((a, b, rv, need(b - a, rv, max_words)))
        a = b
    return out


@dataclass
class MaskContours:
    """Crack contours of P sized planes (Cascade.mask_contours_sized), on the device: the boundary between set and clear
    pixels as closed rings of lattice points -- pixel (y, x) is the square [x, x + 1] x [y, y + 1] --, foreground on the right, one
    vertex per turn.  Plane p's vertices are xy[vertex_offsets[p] : vertex_offsets[p + 1]], ring after ring; a ring starts at its vertex
    with the smallest (y, x) and a plane's rings are ordered by their starts.  An outer ring's first edge heads east and its signed
    area is positive; a hole's heads south and its area is negative; the areas of a plane sum to its popcount."""
    xy: torch.Tensor                # (total, 2) int16 (x, y)
    ring_start: torch.Tensor        # (total,) uint8, 1 on the first vertex of each ring
    vertex_offsets: torch.Tensor    # (P + 1,) int64
    n_vertices: torch.Tensor        # (P,) int32
    n_rings: torch.Tensor           # (P, 2) int32 (outer rings, holes)
    sizes: list                     # P (h, w) pairs, on the host
    connectivity: int
    status: torch.Tensor            # int32 on the device, non-zero if a plane was refused

    def check(self) -> None:
        """RuntimeError if a plane was refused (synchronises): a plane of more than 2^22 vertices, or bits that were written between
        the count and the emit."""
        if bool(self.status.ne(0).any().item()):
            raise RuntimeError(f"mask_contours_sized: a plane was refused: more than {CONTOUR_MAX_VERTS} vertices, or were the bits written "
                               "while the call ran?")

    def rings(self) -> torch.Tensor:
        """Ring r of the call is xy[rings[r] : rings[r + 1]] -> (R + 1,) int64 on the device (synchronises: R is data)."""
        first = torch.nonzero(self.ring_start, as_tuple=False).reshape(-1)
        return torch.cat([first, torch.full((1,), int(self.xy.shape[0]), dtype=torch.int64, device=first.device)])

    def _host_rings(self):
        """-> per plane the list of its rings as int64 arrays (n, 2); one copy of each of the three tensors."""
        self.check()
        xy, start = self.xy.cpu().numpy().astype(np.int64), self.ring_start.cpu().numpy()
        vo = self.vertex_offsets.cpu().numpy()
        out = []
        for p in range(vo.size - 1):
            a, b = int(vo[p]), int(vo[p + 1])
            cuts = a + np.flatnonzero(start[a:b])
            out.append([xy[c:d] for c, d in zip(cuts, list(cuts[1:]) + [b])])
        return out

    def to_coco(self, holes: bool = True) -> list:
        """On the host: one {"size": [h, w], "polygons": [[x0, y0, x1, y1, ...], ...]} per plane, a ring per polygon -- the list
        `polygons_request` takes and the reference's GenericMask holds as `polygons`.  holes=False drops the rings whose first edge
        heads south.  With holes, `polygons_decode` of each ring as a plane of its own, XORed, is the mask; the OR of one annotation
        fills the holes.  Synchronises."""
        out = []
        for (h, w), rings in zip(self.sizes, self._host_rings()):
            keep = [r for r in rings if holes or r[1, 0] != r[0, 0]]
            out.append({"size": [int(h), int(w)], "polygons": [r.reshape(-1).tolist() for r in keep]})
        return out

    def signed_areas(self) -> list:
        """On the host: per plane the float64 array of its rings' signed areas 1/2 sum(x_k y_k+1 - x_k+1 y_k).  Synchronises."""
        area = lambda r: 0.5 * float((r[:, 0] * np.roll(r[:, 1], -1) - np.roll(r[:, 0], -1) * r[:, 1]).sum())
        return [np.asarray([area(r) for r in rings], dtype=np.float64) for rings in self._host_rings()]


SIMPLIFY_MAX_T = 65535            # the tolerance of a plane in quarter pixels (csrc/simplify_logic.h: SP_MAX_T): 16383.75 px


def simplify_request(contours_or_sizes, *, tolerance=1.0, who: str = "simplify_contours") -> np.ndarray:
    """Every check of the arguments of Cascade.simplify_contours, on the host, before anything is launched (ValueError)
    -> the tolerance of each plane in quarter pixels, int32 (P,).  contours_or_sizes: a MaskContours or its (h, w) pairs, 1 .. 65535
    of them.  tolerance: in pixels, an int or a float >= 0 that is a multiple of 0.25 and at most 16383.75 -- one for all planes or one
    per plane; nothing is rounded, no bools."""
    sizes = contours_or_sizes.sizes if isinstance(contours_or_sizes, MaskContours) else contours_or_sizes
    P = len(_plane_sizes(sizes, who))

    def quarters(v) -> int:
        if not _is_real(v) or not np.isfinite(float(v)) or float(v) * 4.0 != np.floor(float(v) * 4.0):
            raise ValueError(f"{who}: a tolerance must be an int or a float that is a multiple of 0.25 pixels (nothing is rounded), got {v!r}")
        return int(float(v) * 4.0)

    if _is_real(tolerance):
        T = quarters(tolerance)
    elif _is_seq(tolerance) and not isinstance(tolerance, torch.Tensor):
        T = [quarters(v) for v in tolerance]
    else:
        raise ValueError(f"{who}: tolerance must be an int or a float in pixels, or hold one per plane, got {tolerance!r}")
    return _per_plane_ints(who, "tolerance, in quarter pixels,", T, P, 0, SIMPLIFY_MAX_T)


@dataclass
class MaskPolygons:
    """Simplified rings of P sized planes (Cascade.simplify_contours), on the device: of every ring of a MaskContours the
    vertices that Ramer-Douglas-Peucker keeps at the plane's tolerance, in the ring's order and from its start; every vertex of the
    ring lies within the tolerance of the segment between the kept vertices around it.  Plane p's vertices are
    xy[vertex_offsets[p] : vertex_offsets[p + 1]], ring after ring, the rings in the order they had.  A ring left with fewer than three
    vertices is dropped and counted in n_dropped.  Simplification does not keep a ring's first edge, so ring_start says what the ring
    was: 1 on the first vertex of an outer ring, 2 on a hole's."""
    xy: torch.Tensor                # (total, 2) int16 (x, y)
    ring_start: torch.Tensor        # (total,) uint8: 1 on the first vertex of an outer ring, 2 on a hole's, 0 elsewhere
    vertex_offsets: torch.Tensor    # (P + 1,) int64
    n_vertices: torch.Tensor        # (P,) int32
    n_rings: torch.Tensor           # (P, 2) int32 (outer rings, holes) that are left
    n_dropped: torch.Tensor         # (P,) int32 rings that were dropped
    sizes: list                     # P (h, w) pairs, on the host
    tolerance: np.ndarray           # (P,) float64, pixels, on the host
    status: torch.Tensor            # int32 on the device, non-zero if a plane was refused

    def check(self) -> None:
        """RuntimeError if a plane was refused (synchronises): a plane that the contour call had refused, or tables that were written
        while the call ran."""
        if bool(self.status.ne(0).any().item()):
            raise RuntimeError("simplify_contours: a plane was refused: did the contour call refuse it, or were the rings written while the "
                               "call ran?")

    def rings(self) -> torch.Tensor:
        """Ring r of the call is xy[rings[r] : rings[r + 1]] -> (R + 1,) int64 on the device (synchronises: R is data)."""
        first = torch.nonzero(self.ring_start, as_tuple=False).reshape(-1)
        return torch.cat([first, torch.full((1,), int(self.xy.shape[0]), dtype=torch.int64, device=first.device)])

    def _host_rings(self):
        """-> per plane the list of its rings as (int64 array (n, 2), whether it is a hole); one copy of each of the three tensors."""
        self.check()
        xy, start = self.xy.cpu().numpy().astype(np.int64), self.ring_start.cpu().numpy()
        vo = self.vertex_offsets.cpu().numpy()
        out = []
        for p in range(vo.size - 1):
            a, b = int(vo[p]), int(vo[p + 1])
            cuts = a + np.flatnonzero(start[a:b])
            out.append([(xy[c:d], int(start[c]) == 2) for c, d in zip(cuts, list(cuts[1:]) + [b])])
        return out

    def to_coco(self, holes: bool = True) -> list:
        """On the host: one {"size": [h, w], "polygons": [[x0, y0, x1, y1, ...], ...]} per plane, a ring per polygon -- the list
        `polygons_request` takes.  holes=False drops the rings that ring_start marks 2.  Synchronises."""
        return [{"size": [int(h), int(w)], "polygons": [r.reshape(-1).tolist() for r, hole in rings if holes or not hole]}
                for (h, w), rings in zip(self.sizes, self._host_rings())]

    def signed_areas(self) -> list:
        """On the host: per plane the float64 array of its rings' signed areas 1/2 sum(x_k y_k+1 - x_k+1 y_k).  Synchronises."""
        area = lambda r: 0.5 * float((r[:, 0] * np.roll(r[:, 1], -1) - np.roll(r[:, 0], -1) * r[:, 1]).sum())
        return [np.asarray([area(r) for r, _ in rings], dtype=np.float64) for rings in self._host_rings()]


DISTANCE_FAR = hip.DT_FAR        # D2 of a pixel with no set pixel within reach
DISTANCE_MAX_REACH = 23170        # a reach and a tolerance radius: 0 .. 23170, 23170^2 < 2^31 (DT_MAX_REACH)
SURFACE_MAX_T = 8                 # tolerances of one Cascade.mask_surface_distances call (DT_MAX_T)
SURFACE_RATIO = 0.008             # the tolerance of the published boundary F-measure: this share of the image's diagonal
SURFACE_MAX_PAIRS = 1 << 24


def surface_tolerance(h: int, w: int, ratio: float = SURFACE_RATIO) -> int:
    """The tolerance radius of an h x w image, in float64: ceil(ratio * diagonal) for a ratio below 1 -- the published
    boundary F-measure's bound_th -- and ceil(ratio) for a ratio that is a pixel count already.  (480, 640) -> 7, (1024, 1024) -> 12,
    (1, 1) -> 1."""
    return int(np.ceil(ratio * np.sqrt(h ** 2 + w ** 2))) if ratio < 1 else int(np.ceil(ratio))


def distance_request(sizes, *, reach=None, who: str = "mask_distance_sized"):
    """Every check of the arguments of Cascade.mask_distance_sized, on the host, before anything is launched
    (ValueError) -> (the (h, w) pairs as ints, the reach of each plane as int32 (P,)).  sizes: 1 .. 65535 pairs of ints in [1, 16384];
    reach: None or 0 for an unlimited search, or an int in [1, 23170] -- for all planes or one per plane -- beyond which a pixel is
    far; no bools."""
    sizes = _plane_sizes(sizes, who)
    return sizes, _per_plane_ints(who, "reach", reach, len(sizes), 0, DISTANCE_MAX_REACH, none=True)


@dataclass
class SurfaceRequest:
    """What `surface_request` hands to Cascade.mask_surface_distances: host tables."""
    a_sizes: list
    b_sizes: list
    pairs: np.ndarray               # (N, 2) int32 (plane of a, plane of b)
    radii: np.ndarray               # (N, T) int32, the tolerance radii of each pair
    reach_a: np.ndarray             # (Pa,) int32, the reach of each plane of a's map (read by the pixels of b)
    reach_b: np.ndarray             # (Pb,) int32


def surface_request(a_sizes, b_sizes, *, pairs=None, tolerance=SURFACE_RATIO, reach=None, who: str = "mask_surface_distances") -> SurfaceRequest:
    """Every check of the arguments of Cascade.mask_surface_distances, on the host, before anything is launched
    (ValueError).  a_sizes / b_sizes: 1 .. 65535 pairs of ints in [1, 16384] each.  pairs: (N, 2) ints (plane of a, plane of b), in
    range and of equal sizes, 1 <= N <= 2^24; None: plane p of a against plane p of b.  tolerance: one tolerance or 1 .. 8 of them,
    each an int in [0, 23170] -- pixels -- or a real in (0, 1) -- a share of the pair's diagonal, `surface_tolerance` --; no bools.
    reach: None -- unlimited --, an int in [0, 23170] for every plane, or "tolerance": each plane's reach is the largest radius of the
    pairs that name it (1 at least), the cheap path when only NSD and F are wanted."""
    is_ratio = lambda v: isinstance(v, (float, np.floating))          # an int is a pixel count, whatever its value
    a_sizes, b_sizes = _plane_sizes(a_sizes, who, "a's sizes"), _plane_sizes(b_sizes, who, "b's sizes")
    Pa, Pb = len(a_sizes), len(b_sizes)
    if pairs is None:
        arr = _plane_by_plane(who, Pa, Pb)
    else:
        if isinstance(pairs, (str, bytes)) or isinstance(pairs, torch.Tensor) and pairs.is_cuda:
            raise ValueError(f"{who}: pairs must be (N, 2) ints on the host")
        try:
            arr = np.asarray(pairs)
        except Exception as e:
            raise ValueError(f"{who}: pairs must be (N, 2) ints") from e
        if arr.ndim != 2 or arr.shape[1] != 2 or arr.dtype.kind not in "iu" or not 1 <= arr.shape[0] <= SURFACE_MAX_PAIRS:
            raise ValueError(f"{who}: pairs must be (N, 2) ints, 1 <= N <= 2^24")
        if bool((arr < 0).any()) or bool((arr[:, 0] >= Pa).any()) or bool((arr[:, 1] >= Pb).any()):
            raise ValueError(f"{who}: a pair names a plane outside [0, {Pa}) x [0, {Pb})")
    arr = np.ascontiguousarray(arr.astype(np.int32))
    dims_a, dims_b = np.asarray(a_sizes, dtype=np.int64)[arr[:, 0]], np.asarray(b_sizes, dtype=np.int64)[arr[:, 1]]
    if bool((dims_a != dims_b).any()):
        i = int(np.nonzero((dims_a != dims_b).any(axis=1))[0][0])
        raise ValueError(f"{who}: pair {i} holds planes of different sizes, {tuple(dims_a[i])} and {tuple(dims_b[i])}")
    tols = [tolerance] if _is_int(tolerance) or is_ratio(tolerance) else tolerance
    if not _is_seq(tols) or not 1 <= len(tols) <= SURFACE_MAX_T:
        raise ValueError(f"{who}: tolerance must be one tolerance or 1 .. {SURFACE_MAX_T} of them, got {tolerance!r}")
    radii = np.empty((arr.shape[0], len(tols)), dtype=np.int32)
    for k, t in enumerate(tols):
        if _is_int(t) and 0 <= int(t) <= DISTANCE_MAX_REACH:
            radii[:, k] = int(t)
        elif is_ratio(t) and 0.0 < float(t) < 1.0:
            radii[:, k] = [surface_tolerance(int(h), int(w), float(t)) for h, w in dims_a]
        else:
            raise ValueError(f"{who}: a tolerance must be an int in [0, {DISTANCE_MAX_REACH}] or a ratio in (0, 1), got {t!r}")
    if isinstance(reach, str) and reach == "tolerance":
        top = radii.max(axis=1)
        reach_a, reach_b = np.ones(Pa, dtype=np.int32), np.ones(Pb, dtype=np.int32)
        np.maximum.at(reach_a, arr[:, 0], top)
        np.maximum.at(reach_b, arr[:, 1], top)
    elif reach is None or _is_int(reach):
        reach_a, reach_b = (_per_plane_ints(who, "reach", reach, P, 0, DISTANCE_MAX_REACH, none=True) for P in (Pa, Pb))
    else:
        raise ValueError(f"{who}: reach must be None, an int in [0, {DISTANCE_MAX_REACH}] or 'tolerance', got {reach!r}")
    return SurfaceRequest(a_sizes=a_sizes, b_sizes=b_sizes, pairs=arr, radii=radii, reach_a=reach_a, reach_b=reach_b)


def surface_rounds(pairs: np.ndarray, a_sizes, b_sizes, cap: int) -> list:
    """The rounds of Cascade.mask_surface_distances: consecutive pairs [i0, i1) taken while the maps of the planes they name -- 6 bytes
    per pixel: 4 of the map, 2 of the distance entry's workspace -- stay within `cap` bytes on either side, one pair at least ->
    [(i0, i1, the planes of a they name, the planes of b, bytes)], the planes sorted.  Pure host arithmetic."""
    px_a = [6 * h * w for h, w in a_sizes]
    px_b = [6 * h * w for h, w in b_sizes]
    out, i0, N = [], 0, len(pairs)
    while i0 < N:
        ua, ub, na, nb, i1 = set(), set(), 0, 0, i0
        while i1 < N:
            p, q = int(pairs[i1, 0]), int(pairs[i1, 1])
            ma, mb = na + (0 if p in ua else px_a[p]), nb + (0 if q in ub else px_b[q])
            if i1 > i0 and max(ma, mb) > cap:
                break
            ua.add(p)
            ub.add(q)
            na, nb, i1 = ma, mb, i1 + 1
        out.append((i0, i1, sorted(ua), sorted(ub), max(na, nb)))
        i0 = i1
    return out


@dataclass
class MaskDistances:
    """Squared distance maps of P sized planes (Cascade.mask_distance_sized), on the device: d2[pix_offsets[p] + y * w + x]
    is the squared distance, between pixel centres, from pixel (y, x) of plane p to the plane's nearest set pixel -- exact, 0 on a set
    pixel, DISTANCE_FAR where none lies within the plane's reach (everywhere on an empty plane)."""
    d2: torch.Tensor                # (total pixels,) int32
    pix_offsets: torch.Tensor       # (P + 1,) int64, in pixels
    sizes: list                     # P (h, w) pairs, on the host
    reach: np.ndarray               # (P,) int32 on the host, 0: unlimited
    status: torch.Tensor            # (1,) int32 on the device, non-zero if a plane was refused

    def check(self) -> None:
        """RuntimeError if the kernel refused a plane (synchronises).  The tables come from the same sizes as the allocation, so this
        says that the input's offsets do not belong to its sizes."""
        if int(self.status.item()) != 0:
            raise RuntimeError("mask_distance_sized: cvlm_mask_distance_sized refused a plane whose slice did not fit its size")

    def plane(self, p: int) -> torch.Tensor:
        """Plane p's map as an int32 view (h, w) of `d2`, from the sizes alone: no read of the device."""
        h, w = self.sizes[p]
        _, off, _ = label_tables(self.sizes)
        return self.d2[int(off[p]):int(off[p + 1])].view(h, w)

    def distance(self, p: int) -> torch.Tensor:
        """Plane p's distances in pixels, float32 (h, w) on the device: the square root, inf where the map is far."""
        m = self.plane(p)
        return torch.where(m == DISTANCE_FAR, torch.full_like(m, float("inf"), dtype=torch.float32), m.to(torch.float32).sqrt())


SURFACE_TABLES = ("n", "far", "within", "max_d2", "sum_d2", "sum_d")


@dataclass
class SurfaceTotals:
    """Directed surface totals of N pairs in both directions (Cascade.mask_surface_distances), on the device.  `ab`: the
    surface pixels of a's plane against the distance map of b's -- prediction against truth --, `ba` the reverse; each a dict of
    n, far, max_d2 int32 (N,), within int32 (N, T), sum_d2 int64 (N,), sum_d float64 (N,).  `surfeval.surface_metrics(to_host())` turns
    them into the Hausdorff distance, ASSD, NSD and the boundary F-measure."""
    pairs: torch.Tensor             # (N, 2) int32
    radii: torch.Tensor             # (N, T) int32, the tolerance radii of each pair
    ab: dict
    ba: dict
    status: torch.Tensor            # (1,) int32, non-zero if a plane or a pair was refused

    def check(self) -> None:
        """RuntimeError if a kernel refused a plane or a pair (synchronises)."""
        if int(self.status.item()) != 0:
            raise RuntimeError("mask_surface_distances: a plane or a pair was refused: do the offsets of the inputs belong to their sizes?")

    def to_host(self) -> dict:
        """Everything as numpy arrays: pairs, radii, status and the two dicts ab / ba (synchronises)."""
        host = lambda d: {k: d[k].cpu().numpy() for k in SURFACE_TABLES}
        return dict(pairs=self.pairs.cpu().numpy(), radii=self.radii.cpu().numpy(), ab=host(self.ab), ba=host(self.ba),
                    status=int(self.status.item()))


THIN_MAX_ITER = hip.THIN_MAX_ITER     # max_iter of a thinning: 1 .. 2^30, None for none
THIN_MAX_STEPS = hip.THIN_MAX_STEPS   # iterations of one round of the stepping path
THIN_PATHS = ("auto", "steps")


def thin_request(sizes, *, max_iter=None, path="auto", steps=64, who: str = "mask_thin_sized"):
    """Every check of the arguments of Cascade.mask_thin_sized, on the host, before anything is launched (ValueError)
    -> (the (h, w) pairs as ints, max_iter of each plane as int32 (P,) with 0 for no limit, the entry's mode, steps).  sizes: 1 .. 65535
    pairs of ints in [1, 16384]; max_iter: None -- thin to the fixed point --, an int in [1, 2^30] for all planes or one such per
    plane; path: "auto" -- a plane that fits the resident kernel's LDS is thinned there, the others in rounds of `steps` stepped
    iterations -- or "steps": every plane is stepped; steps: an int in [1, 1024]; no bools."""
    sizes = _plane_sizes(sizes, who)
    limits = _per_plane_ints(who, "max_iter", max_iter, len(sizes), 1, THIN_MAX_ITER, none=True)
    if not isinstance(path, str) or path not in THIN_PATHS:
        raise ValueError(f"{who}: path must be 'auto' or 'steps', got {path!r}")
    return sizes, limits, THIN_PATHS.index(path), _int_in(who, "steps", steps, 1, THIN_MAX_STEPS)


@dataclass
class MaskThin:
    """Sized planes thinned by Guo & Hall's rule (Cascade.mask_thin_sized), on the device."""
    masks: "SizedMasks"             # the thinned planes: the input's sizes, offsets and level, an area and a box of their own
    iters: torch.Tensor             # (P,) int32: the iterations that cleared at least one pixel
    done: torch.Tensor              # (P,) int32: 1 -- the plane reached its fixed point or its max_iter (every plane of a call that returned)
    status: torch.Tensor            # (1,) int32, non-zero if a plane was refused

    def check(self) -> None:
        """RuntimeError if the kernel refused a plane (synchronises).  The tables come from the same sizes as the allocation, so this
        says that the input's offsets do not belong to its sizes."""
        if int(self.status.item()) != 0:
            raise RuntimeError("mask_thin_sized: cvlm_mask_thin_sized refused a plane whose slice did not fit its size")


CLDICE_TABLES = ("skel_a", "skel_a_in_b", "skel_b", "skel_b_in_a")


@dataclass
class ClDiceTotals:
    """The four counts of centre-line Dice for N pairs (Cascade.mask_cldice), on the device, int32 (N,) each: with S_X
    the plane thinned to its fixed point, skel_a = |S_A|, skel_a_in_b = |S_A & B|, skel_b = |S_B|, skel_b_in_a = |S_B & A|; a pair of
    two different sizes has -1 in both intersections.  `surfeval.cldice(to_host())` turns them into Tprec, Tsens and clDice."""
    pairs: torch.Tensor             # (N, 2) int32 (plane of a, plane of b)
    skel_a: torch.Tensor
    skel_a_in_b: torch.Tensor
    skel_b: torch.Tensor
    skel_b_in_a: torch.Tensor
    status: torch.Tensor            # (1,) int32, non-zero if a plane or a pair was refused

    def check(self) -> None:
        """RuntimeError if a kernel refused a plane or a pair (synchronises)."""
        if int(self.status.item()) != 0:
            raise RuntimeError("mask_cldice: a plane or a pair was refused: two sizes that differ, or offsets that do not belong to the sizes")

    def to_host(self) -> dict:
        """Everything as numpy arrays: pairs, the four counts and status (synchronises)."""
        out = {k: getattr(self, k).cpu().numpy() for k in CLDICE_TABLES}
        return dict(out, pairs=self.pairs.cpu().numpy(), status=int(self.status.item()))


REGIONS_MAXM = hip.REGIONS_MAXM   # regions a plane is split into at most


def regions_request(sizes, *, regions=8, min_area=0, connectivity=8, who: str = "mask_regions_sized"):
    """Every check of the arguments of Cascade.mask_regions_sized, on the host, before anything is launched (ValueError)
    -> (the (h, w) pairs as ints, M, min_area, connectivity).  sizes: 1 .. 65535 pairs of ints in [1, 16384]; regions: an int in
    [1, 64], the slots each plane is split into; min_area: an int in [0, 2^31), regions below it are neither counted nor kept (0 and 1
    keep every region); connectivity: 4 or 8; no bools."""
    sizes = _plane_sizes(sizes, who)
    return (sizes, _int_in(who, "regions", regions, 1, REGIONS_MAXM), _int_in(who, "min_area", min_area, 0, 2 ** 31 - 1),
            _connectivity(who, connectivity))


@dataclass
class MaskRegions:
    """Sized planes split into their connected regions (Cascade.mask_regions_sized), on the device.  Plane p of the
    source has the M slots p * M .. p * M + M - 1 of `masks`, each of plane p's size: slot m holds exactly the pixels of row m of
    `table[p]`, and is an all-zero plane past min(n_regions[p], M)."""
    n_regions: torch.Tensor         # (P,) int32: the regions of at least max(min_area, 1) pixels -- the full count, not capped at M
    table: torch.Tensor             # (P, M, 6) int32 (area, x0, y0, x1, y1, seed), descending area, ties to the lower seed; filler (0, -1 ...)
    masks: "SizedMasks"             # P * M planes in slot order; area and box are the table's columns, the level the source's
    M: int

    def check(self) -> None:
        """RuntimeError if the kernel refused a plane (synchronises).  The tables come from the same sizes as the allocation, so this
        says that the input's offsets do not belong to its sizes."""
        if bool(self.masks.status.ne(0).any().item()):
            raise RuntimeError("mask_regions_sized: cvlm_mask_regions_sized refused a plane whose slice did not fit its size")

    def compact(self):
        """-> (SizedMasks of the real regions only, plane_of, rank): region q of the result is row rank[q] of table[plane_of[q]], in
        slot order; plane_of and rank are host int64 arrays.  The ONE read of the device this feature makes: n_regions and the status,
        together (synchronises; RuntimeError as `check` for a refused plane).  The real slots of a plane lie back to back, so the
        result is one slice of bits, areas and boxes per plane, concatenated on the device -- the style of SizedMasks.concat."""
        P, M, src = int(self.n_regions.shape[0]), self.M, self.masks
        host = torch.cat([self.n_regions.reshape(-1), src.status.reshape(-1).ne(0).any().to(torch.int32).reshape(1)]).cpu().numpy()
        if host[P] != 0:
            raise RuntimeError("mask_regions_sized: cvlm_mask_regions_sized refused a plane whose slice did not fit its size")
        real = np.minimum(host[:P].astype(np.int64), M)
        plane_of = np.repeat(np.arange(P, dtype=np.int64), real)
        rank = np.concatenate([np.arange(r, dtype=np.int64) for r in real]) if P else np.zeros(0, np.int64)
        _, off, _ = src.tables()                                      # of the P * M slots, from the sizes alone
        keep = [p for p in range(P) if real[p] > 0]
        cat = lambda parts, empty: torch.cat(parts) if parts else empty
        bits = cat([src.bits[int(off[p * M]):int(off[p * M + real[p]])] for p in keep], src.bits[:0])
        area = cat([src.area[p * M:p * M + int(real[p])] for p in keep], src.area[:0])
        box = cat([src.box[p * M:p * M + int(real[p])] for p in keep], src.box[:0])
        sizes = [src.sizes[p * M] for p in plane_of]
        offsets = np.zeros(1, np.int64) if not sizes else sized_tables(sizes)[1]
        out = SizedMasks(bits=bits, offsets=_upload(offsets, src.bits.device), area=area, box=box, status=src.status, sizes=sizes, level=src.level)
        return out, plane_of, rank


@dataclass
class RegionClasses:
    """The classes of Q regions (Cascade.classify_regions), on the device."""
    logits: torch.Tensor            # (Q, n_cls) f32
    pred: torch.Tensor              # (Q,) int64 = argmax of logits
    status: torch.Tensor            # int32, one word per chunk: non-zero if cvlm_region_alpha refused a plane or a plane index

    def check(self) -> None:
        """RuntimeError if the kernel refused a region (synchronises)."""
        if bool(self.status.ne(0).any().item()):
            raise RuntimeError("classify_regions: cvlm_region_alpha refused a region whose slice did not fit its size")


def instances_to_coco(rle: "MaskRle", image_ids, category_ids, scores, boxes=None) -> list:
    """COCO result dicts of N instances, on the host, in pure Python: [{"image_id", "category_id", "segmentation", "score"}, ...] with
    `rle.to_coco()`'s rows as segmentations (rle: a MaskRle, or such rows already) -- what COCO.loadRes takes.  image_ids,
    category_ids, scores: one value per instance, sequences or tensors; boxes: optional inclusive (x0, y0, x1, y1) rows, the boxes of
    SizedMasks, written as COCO's "bbox": [x, y, width, height].  ValueError where the lengths differ."""
    rows = rle.to_coco() if isinstance(rle, MaskRle) else list(rle)
    cols = {}
    for name, v in (("image_ids", image_ids), ("category_ids", category_ids), ("scores", scores), ("boxes", boxes)):
        if v is None and name == "boxes":
            continue
        v = v.tolist() if hasattr(v, "tolist") else list(v)
        if len(v) != len(rows):
            raise ValueError(f"instances_to_coco: {name} holds {len(v)} values for {len(rows)} instances")
        cols[name] = v
    out = []
    for i, seg in enumerate(rows):
        d = {"image_id": int(cols["image_ids"][i]), "category_id": int(cols["category_ids"][i]), "segmentation": seg,
             "score": float(cols["scores"][i])}
        if boxes is not None:
            if len(cols["boxes"][i]) != 4:
                raise ValueError(f"instances_to_coco: a box is (x0, y0, x1, y1), got {cols['boxes'][i]!r}")
            x0, y0, x1, y1 = (int(c) for c in cols["boxes"][i])
            d["bbox"] = [x0, y0, x1 - x0 + 1, y1 - y0 + 1]
        out.append(d)
    return out


@dataclass
class MatchRequest:
    """What `match_request` returns: the groups of a COCO matching and the tables cvlm_coco_match takes, on the host."""
    keys: list                      # E (category or None, image id), sorted by (category, image)
    det_perm: np.ndarray            # (sum D,) int64: the caller's detection plane of each row of the detection table, group by group
    gt_perm: np.ndarray             # (sum G,) int64: the same for the annotations
    det_offsets: np.ndarray         # (E + 1,) int32 rows of the detection table
    gt_offsets: np.ndarray          # (E + 1,) int32 rows of the annotation table
    pair_offsets: np.ndarray        # (E + 1,) int64 into pairs
    pairs: np.ndarray               # (N, 2) int32 (the caller's detection plane, annotation plane): group e's D_e x G_e block, detection-major
    crowd: np.ndarray               # (sum G,) uint8 in table order
    range_area: Optional[np.ndarray]    # (sum G,) float64 in table order, the annotation file's "area"; None: the planes' pixel areas
    scores: Optional[np.ndarray]    # (sum D,) float32 in table order when the caller gave them on the host
    iou_thrs: np.ndarray            # (T,) float64
    area_rngs: np.ndarray           # (A, 2) float64
    max_det: int


def match_request(det_sizes, gt_sizes, *, det_image, gt_image, det_category=None, gt_category=None, iscrowd=None, gt_area=None,
                  scores=None, iou_thrs=None, area_rngs=None, max_det=100, who: str = "coco_match") -> MatchRequest:
    """Every check of Cascade.coco_match that the host can make, before anything is launched (ValueError) ->
    MatchRequest.  det_sizes / gt_sizes: the (h, w) of each detection / annotation plane (either list may be empty).  det_image /
    gt_image: one int image id per plane; det_category / gt_category: one int per plane, both or neither -- without them a group is an
    image (pycocotools' useCats = 0).  iscrowd: None or one truth value per annotation; gt_area: None or one finite number >= 0 per
    annotation; scores: None (they are on the device) or one number per detection, no NaN.  iou_thrs: 1 .. 16 numbers in (0, 1], default
    COCO's ten; area_rngs: 1 .. 8 pairs lo <= hi, default all / small / medium / large; max_det: an int >= 1.  All planes of a group have
    one size; a group has at most 1024 detections and 1024 annotations; all groups together at most 2^20 pairs."""
    if not hasattr(det_sizes, "__len__") or not hasattr(gt_sizes, "__len__"):
        raise ValueError(f"{who}: det_sizes and gt_sizes must be sequences of (h, w) pairs")
    Pd, Pg = len(det_sizes), len(gt_sizes)
    ints = lambda name, seq, P: np.asarray(_int_list(who, name, seq, P), dtype=np.int64)

    def reals(name, seq, P, what):
        try:
            arr = np.asarray(seq.cpu() if isinstance(seq, torch.Tensor) else seq)
        except Exception as e:
            raise ValueError(f"{who}: {name} must hold {what}") from e
        if arr.shape != (P,) or (arr.size and arr.dtype.kind not in "iufb"):
            raise ValueError(f"{who}: {name} must hold {what}, {P} of them")
        return arr

    d_img, g_img = ints("det_image", det_image, Pd), ints("gt_image", gt_image, Pg)
    if (det_category is None) != (gt_category is None):
        raise ValueError(f"{who}: give both det_category= and gt_category=, or neither")
    cats = det_category is not None
    d_cat = ints("det_category", det_category, Pd) if cats else np.zeros(Pd, dtype=np.int64)
    g_cat = ints("gt_category", gt_category, Pg) if cats else np.zeros(Pg, dtype=np.int64)
    crowd = np.zeros(Pg, dtype=np.uint8) if iscrowd is None else (reals("iscrowd", iscrowd, Pg, "one truth value per annotation") != 0).astype(np.uint8)
    ra = None
    if gt_area is not None:
        ra = reals("gt_area", gt_area, Pg, "one number per annotation").astype(np.float64)
        if not bool(np.isfinite(ra).all()) or bool((ra < 0).any()):
            raise ValueError(f"{who}: gt_area must be finite and >= 0")
    sc = None
    if scores is not None:
        sc = reals("scores", scores, Pd, "one number per detection").astype(np.float32)
        if bool(np.isnan(sc).any()):
            raise ValueError(f"{who}: a score is NaN")
    try:
        thrs = np.asarray(MATCH_IOU_THRS if iou_thrs is None else iou_thrs, dtype=np.float64)
        rngs = np.asarray(MATCH_AREA_RNGS if area_rngs is None else area_rngs, dtype=np.float64)
    except Exception as e:
        raise ValueError(f"{who}: iou_thrs and area_rngs must hold numbers") from e
    if thrs.ndim != 1 or not 1 <= thrs.size <= MATCH_MAX_T or not bool(((thrs > 0) & (thrs <= 1)).all()):
        raise ValueError(f"{who}: iou_thrs must be 1 .. {MATCH_MAX_T} numbers in (0, 1]")
    if rngs.ndim != 2 or rngs.shape[1] != 2 or not 1 <= rngs.shape[0] <= MATCH_MAX_A or not bool((rngs[:, 0] <= rngs[:, 1]).all()):
        raise ValueError(f"{who}: area_rngs must be 1 .. {MATCH_MAX_A} pairs (lo, hi) with lo <= hi")
    max_det = _int_in(who, "max_det", max_det, 1, 2 ** 31 - 1)
    rows = {}                                                       # (category, image) -> ([detection planes], [annotation planes])
    for side, (cat, img) in enumerate(((d_cat, d_img), (g_cat, g_img))):
        for p, key in enumerate(zip(cat.tolist(), img.tolist())):
            rows.setdefault(key, ([], []))[side].append(p)
    keys = sorted(rows)
    D = [len(rows[k][0]) for k in keys]
    G = [len(rows[k][1]) for k in keys]
    for k, d, g in zip(keys, D, G):
        if d > MATCH_CAP or g > MATCH_CAP:
            raise ValueError(f"{who}: group {k} has {d} detections and {g} annotations, at most {MATCH_CAP} of each are taken")
        sizes = {tuple(det_sizes[p]) for p in rows[k][0]} | {tuple(gt_sizes[q]) for q in rows[k][1]}
        if len(sizes) > 1:
            raise ValueError(f"{who}: the planes of group {k} have the sizes {sorted(sizes)}: one image has one size")
    if not keys:
        raise ValueError(f"{who}: no detection and no annotation")
    n_pairs = int(sum(d * g for d, g in zip(D, G)))
    if n_pairs > 1 << 20:
        raise ValueError(f"{who}: the groups give {n_pairs} pairs, at most 2^20 are taken")
    det_perm = np.asarray([p for k in keys for p in rows[k][0]], dtype=np.int64)
    gt_perm = np.asarray([q for k in keys for q in rows[k][1]], dtype=np.int64)
    blocks = [np.stack(np.meshgrid(rows[k][0], rows[k][1], indexing="ij"), axis=-1).reshape(-1, 2) for k in keys if rows[k][0] and rows[k][1]]
    pairs = np.concatenate(blocks).astype(np.int32) if blocks else np.zeros((0, 2), dtype=np.int32)
    offs = lambda counts, dt: np.concatenate([[0], np.cumsum(counts)]).astype(dt)
    return MatchRequest(keys=[(k[0] if cats else None, k[1]) for k in keys], det_perm=det_perm, gt_perm=gt_perm, det_offsets=offs(D, np.int32),
                        gt_offsets=offs(G, np.int32), pair_offsets=offs([d * g for d, g in zip(D, G)], np.int64),
                        pairs=np.ascontiguousarray(pairs), crowd=crowd[gt_perm], range_area=None if ra is None else ra[gt_perm],
                        scores=None if sc is None else sc[det_perm], iou_thrs=thrs, area_rngs=np.ascontiguousarray(rngs), max_det=max_det)


NMS_MAX_PAIRS = 1 << 22           # pairs of one call (csrc/nms_logic.h: NM_MAX_PAIRS)


@dataclass
class NmsRequest:
    """What `nms_request` returns: the groups of a mask NMS and the tables cvlm_mask_nms_inter / cvlm_mask_nms take, on
    the host."""
    keys: list                      # G image ids, sorted
    member: np.ndarray              # (Q,) int32: the caller's instance of each row of the group table, group by group, in the caller's order
    group_offsets: np.ndarray       # (G + 1,) int32 rows of member
    pair_offsets: np.ndarray        # (G + 1,) int64 into the intersections: group g's D (D - 1) / 2 pairs (i, j), i < j
    thr: float
    measure: int                    # hip.NMS_MEASURES
    method: int                     # hip.NMS_METHODS
    sigma: float

    @property
    def n_pairs(self) -> int:
        return int(self.pair_offsets[-1])


def nms_request(sizes, *, image, iou=0.5, measure="iou", method="greedy", sigma=2.0, who: str = "mask_nms_sized") -> NmsRequest:
    """Every check of Cascade.mask_nms_sized that the host can make, before anything is launched (ValueError) ->
    NmsRequest.  sizes: the (h, w) of each instance plane, 1 .. 65535 of them; image: one int image id per instance -- a group is an
    image, its instances in the caller's order.  iou: the threshold, a number in [0, 1] (an instance is suppressed by a measure strictly
    above it); measure: "iou" or "min" (intersection over the smaller area); method: "greedy", "linear" or "gaussian" (Matrix NMS);
    sigma: a finite number > 0, the gaussian's.  All planes of a group have one size; a group has at most 1024 instances; all groups
    together at most 2^22 pairs.  No bools."""
    sizes = _plane_sizes(sizes, who)
    image = _int_list(who, "image", image, len(sizes), "instance")
    if not _is_real(iou) or not 0.0 <= float(iou) <= 1.0:
        raise ValueError(f"{who}: iou must be a number in [0, 1], got {iou!r}")
    if not isinstance(measure, str) or measure not in hip.NMS_MEASURES:
        raise ValueError(f"{who}: measure must be one of {sorted(hip.NMS_MEASURES)}, got {measure!r}")
    if not isinstance(method, str) or method not in hip.NMS_METHODS:
        raise ValueError(f"{who}: method must be one of {sorted(hip.NMS_METHODS)}, got {method!r}")
    if not _is_real(sigma) or not np.isfinite(float(sigma)) or not float(sigma) > 0.0:
        raise ValueError(f"{who}: sigma must be a finite number > 0, got {sigma!r}")
    rows = {}
    for q, img in enumerate(image):
        rows.setdefault(img, []).append(q)
    keys = sorted(rows)
    for k in keys:
        if len(rows[k]) > MATCH_CAP:
            raise ValueError(f"{who}: image {k} has {len(rows[k])} instances, at most {MATCH_CAP} are taken")
        group_sizes = {sizes[q] for q in rows[k]}
        if len(group_sizes) > 1:
            raise ValueError(f"{who}: the instances of image {k} have the sizes {sorted(group_sizes)}: one image has one size")
    D = [len(rows[k]) for k in keys]
    n_pairs = int(sum(d * (d - 1) // 2 for d in D))
    if n_pairs > NMS_MAX_PAIRS:
        raise ValueError(f"{who}: the groups give {n_pairs} pairs, at most 2^22 are taken")
    offs = lambda counts, dt: np.concatenate([[0], np.cumsum(counts)]).astype(dt)
    return NmsRequest(keys=keys, member=np.asarray([q for k in keys for q in rows[k]], dtype=np.int32), group_offsets=offs(D, np.int32),
                      pair_offsets=offs([d * (d - 1) // 2 for d in D], np.int64), thr=float(iou), measure=hip.NMS_MEASURES[measure],
                      method=hip.NMS_METHODS[method], sigma=float(sigma))


@dataclass
class MaskNms:
    """The NMS of instances across the hypotheses of each image (Cascade.mask_nms_sized; cvlm_mask_nms), on the device.
    Rows are the caller's instances.  Greedy: `keep` is the answer.  Matrix NMS ("linear", "gaussian"): every instance with pixels is
    kept and `rescored(scores)` = scores * decay is what the caller thresholds."""
    keep: torch.Tensor              # (Q,) uint8
    by: torch.Tensor                # (Q,) int32: the instance that suppressed this one, -1 if none
    decay: torch.Tensor             # (Q,) f32: greedy 1 / 0, Matrix NMS the decay coefficient
    order: torch.Tensor             # (Q,) int32: group g's instances by rank at request.group_offsets[g] ..
    n_keep: torch.Tensor            # (G,) int32, the groups in request.keys' order
    inter: torch.Tensor             # (N,) int32: the triangles of cvlm_mask_nms_inter, -1 for a refused pair
    status: torch.Tensor            # (2,) int32: cvlm_mask_nms_inter's and cvlm_mask_nms's -- bit 0 a pair, bit 1 a group was refused
    request: Optional[NmsRequest] = None

    def check(self) -> None:
        """RuntimeError if a kernel refused a pair or a group (synchronises).  The tables come from the same sizes as the instances, so
        this says that the instances' offsets or boxes do not belong to their sizes."""
        if bool(self.status.ne(0).any().item()):
            raise RuntimeError("mask_nms_sized: cvlm_mask_nms_inter or cvlm_mask_nms refused a pair or a group: a slice that does not fit "
                               "its size, or a box outside its plane")

    def rescored(self, scores) -> torch.Tensor:
        """scores * decay -> f32 (Q,) on the device of `decay`: Matrix NMS' new scores (greedy: the kept ones, 0 elsewhere)."""
        s = scores if isinstance(scores, torch.Tensor) else torch.as_tensor(np.asarray(scores, dtype=np.float32))
        if tuple(s.shape) != tuple(self.decay.shape):
            raise ValueError(f"MaskNms.rescored: scores must hold one number per instance, {int(self.decay.numel())} of them")
        return s.detach().to(device=self.decay.device, dtype=torch.float32) * self.decay

    def select(self, instances: "SizedMasks"):
        """-> (SizedMasks of the kept instances in the caller's order, their rows as a host int64 array).  The ONE read of the device
        this feature makes: keep and status, in one tensor (synchronises; RuntimeError as `check`).  Kept neighbours lie back to back,
        so the result is one slice of bits per run of kept rows, by byte ranges from the sizes alone -- the style of
        MaskRegions.compact."""
        Q = int(self.keep.numel())
        if not isinstance(instances, SizedMasks) or len(instances.sizes) != Q or instances.area is None:      # as the call took them: Q may be 0
            raise ValueError(f"MaskNms.select: instances must be the SizedMasks of the call, {Q} planes with areas")
        host = torch.cat([self.status.reshape(-1).view(torch.uint8), self.keep.reshape(-1)]).cpu().numpy()
        n_status = 4 * int(self.status.numel())
        if host[:n_status].any():
            raise RuntimeError("mask_nms_sized: cvlm_mask_nms_inter or cvlm_mask_nms refused a pair or a group: a slice that does not fit "
                               "its size, or a box outside its plane")
        idx = np.flatnonzero(host[n_status:]).astype(np.int64)
        _, off, _ = instances.tables() if Q else (None, np.zeros(1, np.int64), 0)
        starts = [int(q) for k, q in enumerate(idx) if k == 0 or idx[k - 1] != q - 1]
        ends = [int(q) + 1 for k, q in enumerate(idx) if k + 1 == idx.size or idx[k + 1] != q + 1]
        cat = lambda parts, empty: torch.cat(parts) if parts else empty
        bits = cat([instances.bits[int(off[a]):int(off[b])] for a, b in zip(starts, ends)], instances.bits[:0])
        area = cat([instances.area[a:b] for a, b in zip(starts, ends)], instances.area[:0])
        box = cat([instances.box[a:b] for a, b in zip(starts, ends)], instances.box[:0])
        sizes = [instances.sizes[int(q)] for q in idx]
        offsets = np.zeros(1, np.int64) if not sizes else sized_tables(sizes)[1]
        out = SizedMasks(bits=bits, offsets=_upload(offsets, instances.bits.device), area=area, box=box, status=instances.status, sizes=sizes,
                         level=instances.level)
        return out, idx


RENDER_MAX_IMAGES = 65535         # images of one render: the size lists of this module hold 65535 (the entry takes 2^16)
RENDER_MAX_LAYERS = 1 << 20       # layers of one render (RD_MAX_L)
RENDER_MAX_ROWS = 1 << 24         # rows of its colour table (RD_MAX_T)


def image_tables(sizes):
    """Host tables of interleaved 3-channel uint8 images for a list of per-image (h, w): dims int32 (B, 2), byte offsets
    int64 (B + 1) -- image b is its 3 h w bytes, row pitch 3 w, followed by the 0 .. 3 pad bytes that bring the next image to a multiple
    of 4 -- and the largest image's pixel count."""
    dims = np.asarray(sizes, dtype=np.int32).reshape(-1, 2)
    pixels = dims[:, 0].astype(np.int64) * dims[:, 1].astype(np.int64)
    offsets = np.zeros(dims.shape[0] + 1, dtype=np.int64)
    np.cumsum((3 * pixels + 3) // 4 * 4, out=offsets[1:])
    return dims, offsets, int(pixels.max()) if len(pixels) else 0


@dataclass
class SizedImages:
    """Interleaved 3-channel uint8 images, each at its own size, in one flat buffer (`sized_images`): what
    Cascade.render paints on.  Image b is its 3 h w bytes from byte offsets[b] of `data` on; the channel order is the caller's."""
    data: torch.Tensor              # (total bytes,) uint8
    offsets: torch.Tensor           # (B + 1,) int64 in bytes, multiples of 4, on the device of data
    dims: torch.Tensor              # (B, 2) int32 (h, w), on the device of data
    sizes: list                     # B (h, w) pairs, on the host

    def byte_range(self, b: int) -> Tuple[int, int]:
        """Where image b's 3 h w bytes lie in `data`, from the sizes alone: no read of the device."""
        _, offsets, _ = image_tables(self.sizes)
        h, w = self.sizes[b]
        return int(offsets[b]), int(offsets[b]) + 3 * h * w

    def image(self, b: int) -> torch.Tensor:
        """Image b as a uint8 view (h, w, 3) of `data`."""
        lo, hi = self.byte_range(b)
        return self.data[lo:hi].view(*self.sizes[b], 3)

    def to_numpy(self, b: int) -> np.ndarray:
        """Image b as a uint8 array (h, w, 3) on the host (synchronises)."""
        return self.image(b).cpu().numpy()


def sized_images(images, device) -> SizedImages:
    """A list of (h, w, 3) uint8 numpy arrays or tensors -> SizedImages on `device`: the host images go up in one copy of the flat buffer,
    images that are tensors on a device are copied into their slices.  ValueError for anything else; the pad bytes are 0."""
    if isinstance(images, (np.ndarray, torch.Tensor)) or not hasattr(images, "__len__") or not 1 <= len(images) <= RENDER_MAX_IMAGES:
        raise ValueError(f"sized_images: a list of 1 .. {RENDER_MAX_IMAGES} (h, w, 3) uint8 images")
    sizes = []
    for b, im in enumerate(images):
        ok = isinstance(im, (np.ndarray, torch.Tensor)) and im.ndim == 3 and int(im.shape[2]) == 3 and \
            im.dtype in (np.uint8, torch.uint8) and 1 <= int(im.shape[0]) <= SIZED_MAX_SIDE and 1 <= int(im.shape[1]) <= SIZED_MAX_SIDE
        if not ok:
            raise ValueError(f"sized_images: image {b} must be a uint8 array or tensor (h, w, 3) with 1 <= h, w <= {SIZED_MAX_SIDE}")
        sizes.append((int(im.shape[0]), int(im.shape[1])))
    dims, offsets, _ = image_tables(sizes)
    flat = np.zeros(int(offsets[-1]), dtype=np.uint8)
    for b, im in enumerate(images):
        if not (isinstance(im, torch.Tensor) and im.is_cuda):
            host = im.detach().numpy() if isinstance(im, torch.Tensor) else im
            flat[int(offsets[b]):int(offsets[b]) + host.size] = np.ascontiguousarray(host).reshape(-1)
    dev = torch.device(device)
    data = _upload(flat, dev)
    for b, im in enumerate(images):
        if isinstance(im, torch.Tensor) and im.is_cuda:
            data[int(offsets[b]):int(offsets[b]) + im.numel()] = im.detach().to(dev).reshape(-1)
    return SizedImages(data=data, offsets=_upload(offsets, dev), dims=_upload(dims, dev), sizes=sizes)


def palette(n: int) -> np.ndarray:
    """A deterministic colour table, uint8 (n, 3), by the well-known bit-interleave rule: bits 0, 1 and 2 of the id feed r, g and b from
    the top bit down, three bits of the id per round -- 0 black, 1 (128, 0, 0), 2 (0, 128, 0), 3 (128, 128, 0), 4 (0, 0, 128), ..., 15
    (192, 128, 128), ..., 255 (224, 224, 192); ids from 256 on repeat the table."""
    n = _int_in("palette", "n", n, 1, RENDER_MAX_ROWS)
    ids = np.arange(n, dtype=np.int64) & 255
    out = np.zeros((n, 3), dtype=np.uint8)
    for j in range(8):
        for ch in range(3):
            out[:, ch] |= (((ids >> (3 * j + ch)) & 1) << (7 - j)).astype(np.uint8)
    return out


@dataclass
class RenderLayer:
    """One layer of a render, on the host but for its source: what `fill`, `heat` and `classes` build."""
    kind: int                       # hip.RENDER_KINDS
    flags: int                      # hip.RENDER_EDGES (labels), hip.RENDER_INVERT (bits)
    source: torch.Tensor            # the flat buffer the layer reads: packed bits uint8, levels uint8 or labels int32
    src: int                        # where its plane or map starts: bytes (bits, levels) or elements (labels)
    size: Tuple[int, int]           # the (h, w) of that plane or map: the size of the image it may be painted on
    rgb: np.ndarray                 # (rows, 3) the colour of each table row
    alpha: np.ndarray               # (rows,) the opacity of each table row


def _render_colors(who: str, name: str, v, n: Optional[int]) -> np.ndarray:
    """Colours checked -> uint8 (n, 3): ints in 0 .. 255, no bools, no floats; n None: any number of rows >= 1."""
    try:
        arr = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)
    except Exception:
        arr = np.asarray(None)
    if arr.dtype.kind not in "iu" or arr.ndim != 2 or arr.shape[1] != 3 or arr.shape[0] < 1 or (n is not None and arr.shape[0] != n):
        raise ValueError(f"{who}: {name} must hold {'rows' if n is None else n} x 3 ints in 0 .. 255")
    if int(arr.min()) < 0 or int(arr.max()) > 255:
        raise ValueError(f"{who}: {name} must hold ints in 0 .. 255")
    return np.ascontiguousarray(arr.astype(np.uint8))


def _render_alphas(who: str, v, n: int) -> np.ndarray:
    """Opacities checked -> f32 (n,): one finite real in [0, 1] for all rows or one per row; no bools."""
    try:
        arr = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)
    except Exception:
        arr = np.asarray(None)
    if arr.dtype.kind not in "iuf" or arr.shape not in ((), (n,)):
        raise ValueError(f"{who}: alpha must be a real in [0, 1] or hold one per row, {n} of them")
    arr = np.broadcast_to(arr.astype(np.float32), (n,))
    if not bool(np.all(np.isfinite(arr))) or float(arr.min()) < 0.0 or float(arr.max()) > 1.0:
        raise ValueError(f"{who}: an alpha must be finite and in [0, 1]")
    return np.ascontiguousarray(arr)


def _render_index(who: str, name: str, v, n: int) -> int:
    if not _is_int(v) or not 0 <= int(v) < n:
        raise ValueError(f"{who}: {name} must be an int in [0, {n}), got {v!r}")
    return int(v)


def fill(sized: "SizedMasks", p: int, *, color, alpha=0.5, invert: bool = False) -> RenderLayer:
    """A BITS layer: plane p of a SizedMasks painted in one colour at one opacity where its bit is set -- invert=True: where it is
    clear.  Only host rows are built; the plane stays where it is."""
    if not isinstance(sized, SizedMasks) or not isinstance(invert, (bool, np.bool_)):
        raise ValueError("fill: sized must be a SizedMasks and invert a bool")
    p = _render_index("fill", "p", p, len(sized.sizes))
    return RenderLayer(kind=hip.RENDER_KINDS["bits"], flags=hip.RENDER_INVERT if invert else 0, source=sized.bits, src=sized.byte_range(p)[0],
                       size=tuple(int(v) for v in sized.sizes[p]), rgb=_render_colors("fill", "color", [color] if np.ndim(color) == 1 else color, 1),
                       alpha=_render_alphas("fill", alpha, 1))


def heat(levels_u8: torch.Tensor, b: int, *, lut, alpha) -> RenderLayer:
    """A LEVELS layer: map b of a uint8 tensor (N, h, w) or (N, 1, h, w) -- e.g. `mask_to_u8`'s soft masks -- painted through a 256-row
    look-up table of colours at one opacity or one per level (an alpha-0 level leaves its pixels alone)."""
    if not isinstance(levels_u8, torch.Tensor) or levels_u8.dtype != torch.uint8 or levels_u8.dim() not in (3, 4) or \
            (levels_u8.dim() == 4 and levels_u8.shape[1] != 1) or not levels_u8.is_contiguous():
        raise ValueError("heat: levels must be a contiguous uint8 tensor (N, h, w) or (N, 1, h, w)")
    h, w = int(levels_u8.shape[-2]), int(levels_u8.shape[-1])
    b = _render_index("heat", "b", b, int(levels_u8.shape[0]))
    return RenderLayer(kind=hip.RENDER_KINDS["levels"], flags=0, source=levels_u8.detach().view(-1), src=b * h * w, size=(h, w),
                       rgb=_render_colors("heat", "lut", lut, 256), alpha=_render_alphas("heat", alpha, 256))


def classes(label_map: torch.Tensor, label_maps, b: int, *, palette, alpha=0.7, edges: bool = False) -> RenderLayer:
    """A LABELS layer: image b of a flat int32 map of `label_maps` (a LabelMaps: what its `categories()` and `panoptic()` return)
    painted with palette[id] for ids in [0, len(palette)), every other id void; edges=True: only the pixels with a 4-neighbour of
    another id -- the segment outlines."""
    sizes = getattr(label_maps, "sizes", None)
    if not isinstance(sizes, (list, tuple)) or not isinstance(edges, (bool, np.bool_)):
        raise ValueError("classes: label_maps must be the LabelMaps of the map and edges a bool")
    _, offsets, _ = label_tables(sizes)
    if not isinstance(label_map, torch.Tensor) or label_map.dtype != torch.int32 or not label_map.is_contiguous() or \
            label_map.numel() != int(offsets[-1]):
        raise ValueError(f"classes: the map must be a contiguous int32 tensor of the label maps' {int(offsets[-1])} pixels")
    b = _render_index("classes", "b", b, len(sizes))
    rgb = _render_colors("classes", "palette", palette, None)
    return RenderLayer(kind=hip.RENDER_KINDS["labels"], flags=hip.RENDER_EDGES if edges else 0, source=label_map.detach().view(-1),
                       src=int(offsets[b]), size=tuple(int(v) for v in sizes[b]), rgb=rgb, alpha=_render_alphas("classes", alpha, rgb.shape[0]))


@dataclass
class RenderRequest:
    """What `render_request` returns: the tables cvlm_render takes, on the host, and the source buffers the layers name."""
    layer_offsets: np.ndarray       # (B + 1,) int32 rows of layers
    layers: np.ndarray              # (L, 4) int64: kind | flags << 8, src (shifted to its place among the sources of its kind), first, rows
    rgb: np.ndarray                 # (T, 3) uint8
    alpha: np.ndarray               # (T,) f32
    sources: dict                   # kind -> the distinct flat tensors of that kind in the order of their first use: cat gives the buffer

    @property
    def L(self) -> int:
        return int(self.layers.shape[0])


def render_request(sizes, layers, *, device=None, who: str = "render") -> RenderRequest:
    """Every check of Cascade.render that the host can make, before anything is launched (ValueError) -> RenderRequest.
    sizes: the (h, w) of each image; layers: one sequence of RenderLayers per image, in painter's order (an empty one: the image is
    copied).  A layer's plane or map has the size of the image it is painted on and lies inside its source; colours are ints in 0 ..
    255; alphas are finite and in [0, 1]; a LUT has 256 rows; sources live on `device`; at most 2^20 layers and 2^24 table rows."""
    sizes = _plane_sizes(sizes, who)                                  # 65535 at most: RENDER_MAX_IMAGES
    B = len(sizes)
    if isinstance(layers, RenderLayer) or not _is_seq(layers) or len(layers) != B or \
            any(isinstance(ls, (str, bytes, RenderLayer)) or not hasattr(ls, "__iter__") for ls in layers):
        raise ValueError(f"{who}: layers must hold one sequence of layers per image, {B} of them")
    rows, rgb, alpha, counts = [], [], [], []
    sources = {k: [] for k in hip.RENDER_KINDS.values()}
    bases = {k: {} for k in hip.RENDER_KINDS.values()}
    ends = {k: 0 for k in hip.RENDER_KINDS.values()}
    T = 0
    for b, ls in enumerate(layers):
        ls = list(ls)
        counts.append(len(ls))
        for q in ls:
            if not isinstance(q, RenderLayer) or q.kind not in sources or not isinstance(q.source, torch.Tensor) or q.source.dim() != 1:
                raise ValueError(f"{who}: image {b}: a layer must be what fill, heat or classes built")
            if tuple(q.size) != sizes[b]:
                raise ValueError(f"{who}: image {b} is {sizes[b]}, a layer's plane is {tuple(q.size)}")
            h, w = sizes[b]
            kind = q.kind
            names = {v: k for k, v in hip.RENDER_KINDS.items()}
            n_rows = {0: 1, 1: 256}.get(kind)
            q_rgb = _render_colors(who, "a layer's colours", q.rgb, n_rows)
            q_alpha = _render_alphas(who, q.alpha, q_rgb.shape[0])
            allowed = {0: hip.RENDER_INVERT, 1: 0, 2: hip.RENDER_EDGES}[kind]
            need = {0: 4 * h * ((w + 31) // 32), 1: h * w, 2: h * w}[kind]
            dtype = torch.int32 if kind == 2 else torch.uint8
            if q.flags & ~allowed or q.source.dtype != dtype or not isinstance(q.src, (int, np.integer)) or q.src < 0 or \
                    int(q.src) + need > q.source.numel() or (kind == 0 and (q.src % 4 or q.source.numel() % 4)):
                raise ValueError(f"{who}: image {b}: a {names[kind]} layer's flags, source or slice do not fit")
            if device is not None and q.source.device != torch.device(device):
                raise ValueError(f"{who}: image {b}: a layer's source lives on {q.source.device}, the images on {device}")
            key = (q.source.data_ptr(), q.source.numel())
            if key not in bases[kind]:
                bases[kind][key] = ends[kind]
                ends[kind] += q.source.numel()
                sources[kind].append(q.source)
            rows.append((kind | q.flags << 8, bases[kind][key] + int(q.src), T, q_rgb.shape[0]))
            rgb.append(q_rgb)
            alpha.append(q_alpha)
            T += q_rgb.shape[0]
    if len(rows) > RENDER_MAX_LAYERS or T > RENDER_MAX_ROWS:
        raise ValueError(f"{who}: {len(rows)} layers with {T} table rows: at most 2^20 layers and 2^24 rows are taken")
    return RenderRequest(layer_offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                         layers=np.asarray(rows, dtype=np.int64).reshape(-1, 4),
                         rgb=np.concatenate(rgb) if rgb else np.zeros((1, 3), np.uint8),
                         alpha=np.concatenate(alpha) if alpha else np.zeros(1, np.float32), sources=sources)


@dataclass
class Rendered(SizedImages):
    """The images of Cascade.render with their layers painted: a SizedImages plus the kernel's status."""
    status: Optional[torch.Tensor] = None     # (1,) int32: bit 0 an image was refused, bit 1 a layer skipped, bit 2 a refused table row

    def check(self) -> None:
        """RuntimeError if the kernel refused an image, a layer or a table row (synchronises).  `render_request` has checked everything
        on the host, so this says that a source's bytes do not belong to its sizes, or that the library is broken."""
        if bool(self.status.ne(0).any().item()):
            raise RuntimeError(f"render: cvlm_render refused an image (1), a layer (2) or a table row (4): status {int(self.status.item())}")


@dataclass
class CocoMatches:
    """The COCO matching of detections and annotations (Cascade.coco_match; cvlm_coco_match), on the device.  Rows are
    those of the request's tables: group e = request.keys[e] has the detection rows det_offsets[e] .. det_offsets[e + 1] - 1, row i is the
    caller's plane det_perm[i]; likewise the annotations.  dt_match / dt_ignore are in RANK order inside each group."""
    dt_order: torch.Tensor          # (sum D,) int32: rank r of group e holds the row of its detection
    dt_match: torch.Tensor          # (A, T, sum D) int32: the annotation row the detection of that rank took, or -1
    dt_ignore: torch.Tensor         # (A, T, sum D) uint8
    gt_match: torch.Tensor          # (A, T, sum G) int32: the detection row that took the annotation, or -1
    gt_ignore: torch.Tensor         # (A, sum G) uint8
    score: torch.Tensor             # (sum D,) float32 in table (not rank) order
    status: torch.Tensor            # (1,) int32, non-zero if the kernel refused a group
    overlaps: Optional["SizedOverlaps"]     # the intersections behind it; None when no group has both detections and annotations
    request: MatchRequest
    boundary_overlaps: Optional["SizedOverlaps"] = None     # coco_match(boundary=...): the intersections of the boundaries

    def check(self) -> None:
        """RuntimeError if the kernel refused a group or a pair (synchronises).  The tables come from `match_request`, so a refused
        group says that the library is broken; a refused pair is two planes whose tables do not fit."""
        if int(self.status.item()) != 0:
            raise RuntimeError("coco_match: cvlm_coco_match refused a group: offsets or a pair block that do not fit")
        for overlaps in (self.overlaps, self.boundary_overlaps):
            if overlaps is not None:
                overlaps.check()

    def to_host(self) -> dict:
        """Everything cocoeval.accumulate needs, as numpy arrays, by ONE read of the device (synchronises): the five result tables under
        their names, `score` in table order, `status`, and the request's `keys`, `det_offsets`, `gt_offsets`, `det_perm`, `gt_perm`,
        `iou_thrs`, `area_rngs`, `max_det`."""
        parts = [self.dt_order, self.dt_match, self.gt_match, self.score, self.status, self.dt_ignore, self.gt_ignore]
        flat = torch.cat([t.contiguous().view(-1).view(torch.uint8) for t in parts]).cpu().numpy()
        out, at = {}, 0
        for name, t in zip(("dt_order", "dt_match", "gt_match", "score", "status", "dt_ignore", "gt_ignore"), parts):
            n = t.numel() * t.element_size()
            dt = {torch.int32: np.int32, torch.float32: np.float32, torch.uint8: np.uint8}[t.dtype]
            out[name] = flat[at:at + n].view(dt).reshape(tuple(t.shape))
            at += n
        r = self.request
        out.update(status=int(out["status"][0]), keys=list(r.keys), det_offsets=r.det_offsets, gt_offsets=r.gt_offsets, det_perm=r.det_perm,
                   gt_perm=r.gt_perm, iou_thrs=r.iou_thrs, area_rngs=r.area_rngs, max_det=r.max_det)
        return out


def ground_truth_request(ground_truth, sreq, n: int, who: str = "decode"):
    """Every check of the ground_truth= argument of Cascade.infer_classes / decode, on the host, before anything is
    launched (ValueError) -> None when nothing is asked for, otherwise (gt, the image id of each of its planes).  ground_truth is (gt,
    gt_image): a SizedMasks with areas -- `rle_decode` of the annotations -- and one id in [0, n) per plane of it, the image of the call
    the annotation belongs to; it needs sizes=, and every gt.sizes[q] must be the size of image gt_image[q]."""
    if ground_truth is None:
        return None
    if not isinstance(ground_truth, (tuple, list)) or len(ground_truth) != 2 or not isinstance(ground_truth[0], SizedMasks):
        raise ValueError(f"{who}: ground_truth must be (SizedMasks, image id of each of its planes)")
    gt, ids = ground_truth
    if sreq is None:
        raise ValueError(f"{who}: ground_truth= is held against the sized planes: give sizes=")
    _sized_arg(who, "the annotations of ground_truth=", gt, areas=True)
    ids = _int_list(who, "the image ids of ground_truth=", ids, len(gt.sizes), "annotation")
    sizes, _ = sreq
    for q, b in enumerate(ids):
        if not 0 <= b < n:
            raise ValueError(f"{who}: annotation {q} names image {b} of {n}")
        if tuple(gt.sizes[q]) != tuple(sizes[b]):
            raise ValueError(f"{who}: annotation {q} is {tuple(gt.sizes[q])}, image {b} is {tuple(sizes[b])}")
    return gt, ids


@dataclass
class SizedOverlaps:
    """Intersections of pairs of sized planes (Cascade.mask_inter_sized, ground_truth= of infer_classes / decode), on the
    device.  Pair i is (plane pairs[i, 0] of a, plane pairs[i, 1] of b); inter[i] = |a AND b| in pixels, -1 for a refused pair (planes
    of different sizes, an index or a table that does not fit)."""
    pairs: torch.Tensor             # (N, 2) int32
    inter: torch.Tensor             # (N,) int32
    area_a: torch.Tensor            # (N,) int32 the area of each pair's plane of a
    area_b: torch.Tensor            # (N,) int32 the area of each pair's plane of b
    status: torch.Tensor            # (1,) int32, non-zero if a pair was refused

    def check(self) -> None:
        """RuntimeError if the kernel refused a pair (synchronises)."""
        if int(self.status.item()) != 0:
            raise RuntimeError("mask_inter_sized: cvlm_mask_inter_sized refused a pair: sizes that differ, an index or a table that does not fit")

    def iou(self, iscrowd=None) -> np.ndarray:
        """The COCO IoU of each pair, float64 (N,), on the host: pycocotools' rleIou.  -1 where inter is -1; 0 where inter is 0;
        inter / area_a where iscrowd[q] is true for the pair's plane q of b (a crowd annotation: the share of the detection inside
        it); inter / (area_a + area_b - inter) otherwise.  iscrowd: None or one truth value per plane of b.  ONE read of the device
        (synchronises)."""
        table = torch.stack([self.pairs[:, 1], self.inter, self.area_a, self.area_b]).cpu().numpy().astype(np.int64)
        q, inter, a, b = table
        crowd = np.zeros(q.shape, dtype=bool)
        if iscrowd is not None:
            flags = np.asarray(iscrowd).astype(bool).reshape(-1)
            ok = (q >= 0) & (q < flags.size)
            crowd[ok] = flags[q[ok]]
        out = np.zeros(q.shape, dtype=np.float64)
        pos = inter > 0
        union = np.where(crowd, a, a + b - inter)
        out[pos] = inter[pos] / union[pos].astype(np.float64)
        out[inter < 0] = -1.0
        return out


def _rows(t: Optional[torch.Tensor], own: int, p0: int, p1: int) -> Optional[torch.Tensor]:
    """Rows p0 .. p1 - 1 of a result tensor whose last `own` dimensions are one hypothesis's: (n, K, ...) seen as (n * K, ...)."""
    return None if t is None else t.view(-1, *t.shape[t.dim() - own:])[p0:p1]


class MaskUtilities:
    """The stand-alone utilities of the packed-mask family, methods of Cascade: each checks its arguments on the host, allocates its
    results and launches on the caller's stream.  Of the engine they use `self.device` and the workspace `self.ws` only."""

    @staticmethod
    def _packed_planes(who: str, bits, H, W):
        """The (bits, H, W) arguments of a utility on packed planes, checked (ValueError) -> (bits, N, H, W): uint8 (N, H * W / 8) on
        the device, W a multiple of 32; detached, contiguous and, where a view starts off a 4-byte boundary, copied (the kernels read
        32-bit words)."""
        if not _is_int(H) or not _is_int(W) or H < 1 or W < 1 or W % 32 != 0 or H * W >= 2 ** 31:
            raise ValueError(f"{who}: planes of {H} x {W}: W must be a multiple of 32 and H * W below 2^31")
        H, W = int(H), int(W)
        if not isinstance(bits, torch.Tensor) or bits.dtype != torch.uint8 or bits.dim() != 2 or int(bits.shape[1]) != H * W // 8 \
                or not 1 <= int(bits.shape[0]) <= 65535:
            raise ValueError(f"{who}: bits must be a uint8 tensor (N, {H * W // 8}) with 1 <= N <= 65535")
        if not bits.is_cuda:
            raise ValueError(f"{who}: bits must be on the device")
        return _aligned(bits), int(bits.shape[0]), H, W

    @staticmethod
    def _f32_planes(who: str, name: str, t, hw: str):
        """The f32 planes of a utility, (N, h, w) or (N, 1, h, w), checked by type and rank (ValueError) -> (N, h, w); `hw` is how the
        message writes the two sides."""
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() not in (3, 4) or (t.dim() == 4 and t.shape[1] != 1):
            raise ValueError(f"{who}: {name} must be a float32 tensor (N, {hw}) or (N, 1, {hw})")
        return int(t.shape[0]), int(t.shape[-2]), int(t.shape[-1])

    # ---- packed masks, areas, boxes and overlaps -----------------------------------------------------------------
    def pack_masks(self, logits: torch.Tensor):
        """(bits, area, box) of any (N, S, S) or (N, 1, S, S) f32 mask logits on this engine's device, e.g. `infer_test`'s: bits uint8
        (N, S * S / 8) = logits > 0 in numpy.packbits' order, area int32 (N,), box int32 (N, 4) inclusive (x0, y0, x1, y1), -1 for an
        empty mask (cvlm_mask_pack).  One launch pair on the caller's stream; ValueError before it for anything else."""
        N, H, W = self._f32_planes("pack_masks", "logits", logits, "H, W")
        if not 1 <= N <= 65535 or H * W < 1 or (H * W) % 32 != 0 or H * W >= 2 ** 31:
            raise ValueError(f"pack_masks: {N} planes of {H} x {W}: 1 .. 65535 planes of a multiple of 32 pixels below 2^31")
        if not logits.is_cuda:
            raise ValueError("pack_masks: logits must be on the device")
        planes = logits.detach().contiguous().view(N, H, W)
        dev = logits.device
        bits, area, box = _empty(dev, N, H * W // 8, dtype=torch.uint8), _empty(dev, N), _empty(dev, N, 4)
        hip.mask_pack(planes, bits, area, box)
        return bits, area, box

    # ---- connected components of packed masks -----------------------------------------------------------------------
    def _component_outputs(self, lead: tuple, nbytes: int, M: int, min_area: int):
        """The result's own (n_comp, comps, n_kept, kept_bits, kept_area, kept_box) for planes of shape `lead`: no table with M = 0, the
        last four only with min_area >= 1."""
        i32 = partial(_empty, self.device, *lead)
        if min_area < 1:
            return i32(), i32(M, 6) if M else None, None, None, None, None
        return i32(), i32(M, 6) if M else None, i32(), i32(nbytes, dtype=torch.uint8), i32(), i32(4)

    def _components(self, bits: torch.Tensor, H: int, W: int, connectivity: int, min_area: int, rows) -> None:
        """cvlm_mask_components of the planes bits (N, H * W / 8) into `rows`, their N rows of the six result tensors.  The workspace
        "cls_comp" grows to what these planes want in flight, up to COMPONENTS_WS_CAP (and never below one plane's)."""
        want = _capped(hip.mask_components_workspace_bytes(int(bits.shape[0]), H, W), hip.mask_components_workspace_bytes(1, H, W), COMPONENTS_WS_CAP)
        hip.mask_components(bits, H, W, connectivity, min_area, self.ws.scratch("cls_comp", want), *rows)

    def mask_components(self, bits: torch.Tensor, H: int, W: int, *, components: Optional[int] = 1, min_area: int = 0,
                        connectivity: int = 8) -> "MaskComponents":
        """Connected regions of any (N, H * W / 8) uint8 packed masks on this engine's device, e.g. `pack_masks`' bits (W % 32 == 0):
        the number of regions, the `components` largest with their boxes and seeds and, with min_area >= 1, the masks without
        their regions below min_area pixels, with area and box (cvlm_mask_components) -> MaskComponents.  Launches
        on the caller's stream; ValueError before them for anything else."""
        _, M, min_area, connectivity = components_request(components=components, min_area=min_area, connectivity=connectivity,
                                                          who="mask_components")
        bits, N, H, W = self._packed_planes("mask_components", bits, H, W)
        out = self._component_outputs((N,), H * W // 8, M, min_area)
        self._components(bits, H, W, connectivity, min_area, out)
        return MaskComponents(*out)

    # ---- holes of packed masks ----------------------------------------------------------------------------------------
    def _hole_outputs(self, lead: tuple, nbytes: int, M: int, fill_below: int):
        """The result's own (n_holes, holes, n_filled, filled_bits, filled_area) for planes of shape `lead`: no table with M = 0, the
        last three only with fill_below >= 1."""
        i32 = partial(_empty, self.device, *lead)
        if fill_below < 1:
            return i32(), i32(M, 6) if M else None, None, None, None
        return i32(), i32(M, 6) if M else None, i32(), i32(nbytes, dtype=torch.uint8), i32()

    def _holes(self, bits: torch.Tensor, H: int, W: int, connectivity: int, fill_below: int, rows) -> None:
        """cvlm_mask_holes of the planes bits (N, H * W / 8) into `rows`, their N rows of the five result tensors.  The workspace is
        `_components`' "cls_comp", grow-only under the same COMPONENTS_WS_CAP: the two entries are ordered on one stream."""
        want = _capped(hip.mask_holes_workspace_bytes(int(bits.shape[0]), H, W), hip.mask_holes_workspace_bytes(1, H, W), COMPONENTS_WS_CAP)
        hip.mask_holes(bits, H, W, connectivity, fill_below, self.ws.scratch("cls_comp", want), *rows)

    def mask_holes(self, bits: torch.Tensor, H: int, W: int, *, holes: Optional[int] = 1, fill_holes: int = 0,
                   connectivity: int = 8) -> "MaskHoles":
        """Holes of any (N, H * W / 8) uint8 packed masks on this engine's device, e.g. `pack_masks`' bits (W % 32 == 0): the number
        of holes, the `holes` largest with their boxes and seeds and, with fill_holes >= 1, the masks with their holes of fewer than
        fill_holes pixels set, with their area (cvlm_mask_holes) -> MaskHoles.  connectivity is the foreground's; the
        clear pixels connect at its dual.  SAM's post-processing, fill then despeckle, is
        mask_components(mask_holes(bits, H, W, fill_holes=t).filled_bits, H, W, min_area=t).  Launches on the caller's stream;
        ValueError before them for anything else."""
        _, M, fill_below, connectivity = holes_request(holes=holes, fill_holes=fill_holes, connectivity=connectivity, who="mask_holes")
        bits, N, H, W = self._packed_planes("mask_holes", bits, H, W)
        out = self._hole_outputs((N,), H * W // 8, M, fill_below)
        self._holes(bits, H, W, connectivity, fill_below, out)
        return MaskHoles(*out)

    # ---- packed edge maps -------------------------------------------------------------------------------------------
    def pack_edges(self, prob: torch.Tensor, size=None, *, threshold: float, with_bits: Optional[torch.Tensor] = None) -> "EdgeBits":
        """Packed edge maps of any (N, h, w) or (N, 1, h, w) f32 probability planes on this engine's device (cvlm_edge_pack, DESIGN.md
        §17) -> EdgeBits: bits uint8 (N, H * W / 8) in numpy.packbits' order, set where the align_corners=False bilinear value at
        size = (H, W) is > threshold, and their area.  size=None means (h, w), a pure threshold pack: that is how
        `infer_test_multimask(...).edges` is packed; a low-resolution map takes size=(S, S).  with_bits: (N, H * W / 8) uint8 packed
        planes, e.g. `mask_morph`'s band_bits: `inter` = |bits AND with_bits| per plane.  0 < threshold < 1, W % 32 == 0.  One launch
        pair on the caller's stream; ValueError before it for anything else."""
        t = _edge_threshold(threshold, "pack_edges")
        N, h, w = self._f32_planes("pack_edges", "prob", prob, "h, w")
        if size is None:
            size = (h, w)
        if not isinstance(size, (tuple, list)) or len(size) != 2 or not all(_is_int(v) for v in size):
            raise ValueError(f"pack_edges: size must be None or a pair of ints (H, W), got {size!r}")
        H, W = (int(v) for v in size)
        if not 1 <= N <= 65535 or h < 1 or w < 1 or h * w >= 2 ** 31 or H < 1 or W < 1 or W % 32 != 0 or H * W >= 2 ** 31:
            raise ValueError(f"pack_edges: {N} planes of {h} x {w} to {H} x {W}: 1 .. 65535 planes, W a multiple of 32, both sizes "
                             "below 2^31 pixels")
        if not prob.is_cuda:
            raise ValueError("pack_edges: prob must be on the device")
        if with_bits is not None:
            if not isinstance(with_bits, torch.Tensor) or with_bits.dtype != torch.uint8 or tuple(with_bits.shape) != (N, H * W // 8):
                raise ValueError(f"pack_edges: with_bits must be a uint8 tensor ({N}, {H * W // 8})")
            if with_bits.device != prob.device:
                raise ValueError("pack_edges: with_bits must be on prob's device")
            with_bits = _aligned(with_bits)
        planes = prob.detach().contiguous().view(N, h, w)
        dev = prob.device
        bits, area = _empty(dev, N, H * W // 8, dtype=torch.uint8), _empty(dev, N)
        inter = _empty(dev, N) if with_bits is not None else None
        hip.edge_pack(planes, H, W, t, bits, area, with_bits, inter)
        return EdgeBits(bits, area, inter)

    # ---- morphology of packed masks -----------------------------------------------------------------------------------
    def mask_morph(self, bits: torch.Tensor, H: int, W: int, *, radius: int = 2, dilate: bool = False, erode: bool = False,
                   band: bool = True) -> "MaskMorph":
        """Dilation, erosion and edge band = dilation & ~erosion of any (N, H * W / 8) uint8 packed masks on this engine's device, e.g.
        `pack_masks`' bits (W % 32 == 0), by the (2 radius + 1)^2 square, 1 <= radius <= 16, each with its area (cvlm_mask_morph,
        DESIGN.md §16) -> MaskMorph, None where an output was not asked for.  Pixels outside the plane are clear to dilation and set to
        erosion, as max_pool2d's padding has it: radius=2 is the band the reference trains its edge head against.  Opening and closing
        are compositions through this utility: opening = mask_morph(mask_morph(bits, ..., erode=True, band=False).ero_bits, ...,
        dilate=True, band=False).dil_bits, closing the reverse; a SAM-style chain is
        mask_components(mask_holes(mask_morph(bits, H, W, dilate=True, band=False).dil_bits, H, W, fill_holes=t).filled_bits, H, W,
        min_area=t).  Launches on the caller's stream; ValueError before them for anything else."""
        radius = _int_in("mask_morph", "radius", radius, 1, MORPH_MAXR)
        for name, v in (("dilate", dilate), ("erode", erode), ("band", band)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"mask_morph: {name} must be a bool, got {type(v).__name__}")
        if not (dilate or erode or band):
            raise ValueError("mask_morph: nothing asked for: at least one of dilate, erode and band")
        bits, N, H, W = self._packed_planes("mask_morph", bits, H, W)
        out = []
        for asked in (dilate, erode, band):
            out += [torch.empty_like(bits), _empty(bits.device, N)] if asked else [None, None]
        hip.mask_morph(bits, H, W, radius, *out)
        return MaskMorph(*out)

    # ---- run-length encoding of packed masks ------------------------------------------------------------------------
    def mask_rle(self, bits: torch.Tensor, H: int, W: int) -> "MaskRle":
        """COCO run-length encoding of any (N, H * W / 8) uint8 packed masks on this engine's device, e.g. `pack_masks`' bits or
        `mask_components`' kept_bits (W % 32 == 0; H any) -> MaskRle.  cvlm_mask_rle_count, torch.cumsum of the run counts on the device,
        ONE device-to-host read of the total -- the call's only synchronisation, and the size of `counts` is known before it is
        allocated --, then cvlm_mask_rle_emit through the grow-only workspace "cls_rle", capped at RLE_WS_CAP (beyond it the entry
        walks the planes in rounds).  The emit's status word stays on the device: `MaskRle.check()` / `to_coco()` read it.  Launches on
        the caller's stream; ValueError before them for anything else."""
        bits, N, H, W = self._packed_planes("mask_rle", bits, H, W)
        dev, i32 = bits.device, partial(_empty, bits.device)
        n_runs = i32(N)
        hip.mask_rle_count(bits, H, W, n_runs)
        offsets = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        torch.cumsum(n_runs, 0, dtype=torch.int64, out=offsets[1:])
        total = int(offsets[N].item())                               # the one synchronisation
        counts, status = i32(total), i32(1)
        want = _capped(hip.mask_rle_workspace_bytes(N, H, W), hip.mask_rle_workspace_bytes(1, H, W), RLE_WS_CAP)
        hip.mask_rle_emit(bits, H, W, offsets, counts, status, self.ws.scratch("cls_rle", want))
        return MaskRle(counts=counts, offsets=offsets, n_runs=n_runs, size=(H, W), status=status)

    # ---- masks at each image's own size ---------------------------------------------------------------------------
    def _sized_outputs(self, sizes, level: int, K: int, n_calls: int):
        """The SizedMasks of K planes per (h, w) of `sizes`, one status word per cvlm_mask_pack_sized call, and the device table of the
        planes' (h, w) -- built on the host and uploaded once -> (SizedMasks, dims, largest word count)."""
        out, dims, max_words = SizedMasks.empty([s for s in sizes for _ in range(K)], self.device, level=level, n_status=n_calls)
        return out, _upload(dims, self.device), max_words

    @staticmethod
    def _pack_sized(planes: torch.Tensor, out: "SizedMasks", dims: torch.Tensor, max_words: int, p0: int, p1: int, call: int) -> None:
        """cvlm_mask_pack_sized of p1 - p0 full-resolution planes into the planes p0 .. p1 - 1 of `out`: one call whatever sizes they
        have, no workspace."""
        hip.mask_pack_sized(planes[:p1 - p0], dims[p0:p1], out.offsets[p0:p1 + 1], out.level, out.bits, max_words, out.area[p0:p1],
                            out.box[p0:p1], out.status[call:call + 1])

    def pack_masks_sized(self, logits: torch.Tensor, sizes, *, level: int = 128) -> "SizedMasks":
        """Packed masks of any (N, Hs, Ws) or (N, 1, Hs, Ws) f32 mask logits on this engine's device at a size of each plane's own:
        sizes holds N (h, w) pairs -> SizedMasks (cvlm_mask_pack_sized).  A bit is set where the reference's uint8 mask
        -- sigmoid, cv2.resize(INTER_LINEAR) to (h, w), * 255 (test_ovcos_maskdecoder_edge.py:103,116-130; demo.py:117-131) -- is >=
        level: 128 is the half, 1 the demo's `> 0` overlay.  At (Hs, Ws) itself the bits are NOT `pack_masks`' (logit > 0): they go
        through the same arithmetic with weights 1 and 0.  One launch pair on the caller's stream whatever the mix of sizes, the two
        small tables uploaded before it; no workspace.  ValueError before anything is launched for anything else."""
        N, Hs, Ws = self._f32_planes("pack_masks_sized", "logits", logits, "H, W")
        if not 1 <= N <= 65535 or Hs < 1 or Ws < 1 or Hs * Ws >= 2 ** 31:
            raise ValueError(f"pack_masks_sized: {N} planes of {Hs} x {Ws}: 1 .. 65535 planes of fewer than 2^31 pixels")
        if not logits.is_cuda:
            raise ValueError("pack_masks_sized: logits must be on the device")
        sreq = sized_request(sizes=sizes, sized_level=level, n=N, who="pack_masks_sized")
        if sreq is None:
            raise ValueError("pack_masks_sized: sizes must be a sequence of (h, w) pairs, got None")
        sizes, level = sreq
        out, dims, max_words = self._sized_outputs(sizes, level, 1, 1)
        self._pack_sized(logits.detach().contiguous().view(N, Hs, Ws), out, dims, max_words, 0, N, 0)
        return out

    # ---- label maps -------------------------------------------------------------------------------------------------
    def _label_outputs(self, sizes, K: int, weights, level: int, overlap_threshold: float):
        """The LabelMaps of K hypotheses per (h, w) of `sizes` with its two tables uploaded, the weights on the device (or None) and
        the largest image's pixel count; cvlm_label_init has written the fill."""
        dims, offsets, max_pixels = label_tables(sizes)
        dev, B, n_pix = self.device, len(sizes), int(offsets[-1])
        i32 = partial(_empty, dev)
        out = LabelMaps(score=i32(n_pix, dtype=torch.float32), winner=i32(n_pix, dtype=torch.int16), segment=i32(n_pix, dtype=torch.int16), areas=i32(3, B * K),
                        segment_id=i32(B * K), n_segments=i32(B), status=i32(1), dims=_upload(dims, dev), pix_offsets=_upload(offsets, dev),
                        sizes=[tuple(s) for s in sizes], K=K, level=level, overlap_threshold=overlap_threshold)
        if isinstance(weights, np.ndarray):
            weights = _upload(weights, dev)
        elif weights is not None:
            weights = weights.detach().contiguous().view(-1)
        hip.label_init(out.score, out.winner, out.segment, out.areas, out.segment_id, out.n_segments, out.status, B, K)
        return out, weights, max_pixels

    @staticmethod
    def _label_accumulate(planes: torch.Tensor, out: "LabelMaps", weights, max_pixels: int, p0: int, p1: int) -> None:
        """cvlm_label_accumulate of the p1 - p0 full-resolution planes p0 .. p1 - 1: one launch, whatever images they belong to."""
        hip.label_accumulate(planes[:p1 - p0], p0, out.B, out.K, out.dims, out.pix_offsets, weights, out.level, out.score, out.winner,
                             out.segment, max_pixels, out.areas, out.status)

    @staticmethod
    def _label_finish(out: "LabelMaps", max_pixels: int) -> None:
        hip.label_finish(out.B, out.K, out.dims, out.pix_offsets, out.overlap_threshold, out.winner, out.segment, max_pixels,
                         out.areas, out.segment_id, out.n_segments, out.status)

    def label_maps(self, logits: torch.Tensor, sizes, *, K: int, weights=None, level: int = 128, overlap_threshold: float = 0.8) -> "LabelMaps":
        """One label map per image from (B * K, Hs, Ws) or (B * K, 1, Hs, Ws) f32 mask logits on this engine's device, plane b * K + k the
        k-th hypothesis of image b, at the B sizes (h, w) of `sizes` -> LabelMaps (cvlm_label_init / accumulate / finish).
        Per pixel the hypothesis with the largest weight * value wins, the value being the reference's resized sigmoid mask as
        `pack_masks_sized` forms it (ties: the smallest k; a NaN plane never wins); per hypothesis Mask2Former's areas and overlap test
        decide which own a segment.  weights: one per hypothesis -- the score that ranks them is the caller's: a softmax of pass-1
        logits at the hypothesis's class, a predicted quality --, None for 1.  Five launches on the caller's stream, the tables
        uploaded before them; no workspace, no synchronisation.  ValueError before anything is launched for anything else."""
        N, Hs, Ws = self._f32_planes("label_maps", "logits", logits, "H, W")
        if not _is_int(K) or K < 1 or N % K != 0:
            raise ValueError(f"label_maps: {N} planes are no whole number of images of K = {K!r} hypotheses")
        B = N // int(K)
        if not 1 <= B <= 65535 or Hs < 1 or Ws < 1 or Hs * Ws >= 2 ** 31:
            raise ValueError(f"label_maps: {B} images of planes of {Hs} x {Ws}: 1 .. 65535 images of fewer than 2^31 pixels")
        sreq = sized_request(sizes=sizes, sized_level=level, n=B, who="label_maps")
        lreq = labels_request(label_maps=True, sizes=sizes, weights=weights, level=level, overlap_threshold=overlap_threshold, n=B, K=int(K),
                              who="label_maps")
        weights, level, overlap_threshold = lreq
        if not logits.is_cuda or (isinstance(weights, torch.Tensor) and weights.device != logits.device):
            raise ValueError("label_maps: logits (and weights given as a device tensor) must be on this engine's device")
        out, weights, max_pixels = self._label_outputs(sreq[0], int(K), weights, level, overlap_threshold)
        self._label_accumulate(logits.detach().contiguous().view(N, Hs, Ws), out, weights, max_pixels, 0, N)
        self._label_finish(out, max_pixels)
        return out

    def label_iou(self, pred, gt, *, num_classes: int, ignore_index: int = 255, reduce_zero_label: bool = False, totals=None) -> torch.Tensor:
        """mmseg's intersect_and_union of a predicted label map against ground truth, summed on the device (cvlm_label_iou_hist, DESIGN.md
        §23) -> totals int64 (3, num_classes) = (area_intersect, area_pred_label, area_label), which `segeval.eval_metrics` turns into
        aAcc, Acc and IoU / Dice.  pred: integers of any shape, e.g. `LabelMaps.categories(classes)`; gt: as many integers, uint8 or
        int32; both on this engine's device, or host arrays that are uploaded.  The kernel reads int32: any other integer type is
        converted, and its values must lie in the int32 range -- a host array is checked (ValueError), a device tensor is the caller's
        contract (a check would synchronise; a value outside the range wraps).  totals: the result
        of an earlier call, accumulated into -- a dataset's batches sum on the device; None starts from zero.  A value outside
        [0, num_classes - 1] is counted nowhere (np.histogram would count the value num_classes in the last class); `label_map` is the
        caller's: remap before upload.  No synchronisation.  ValueError before anything is launched for anything else."""
        C_ = _int_in("label_iou", "num_classes", num_classes, 1, LABELS_MAX_CLASSES)
        ignore_index = _int_in("label_iou", "ignore_index", ignore_index, -2 ** 31, 2 ** 31 - 1)
        if not isinstance(reduce_zero_label, (bool, np.bool_)):
            raise ValueError(f"label_iou: reduce_zero_label must be a bool, got {reduce_zero_label!r}")
        maps = []
        for name, m in (("pred", pred), ("gt", gt)):
            t = _integer_map("label_iou", name, m)
            keep = name == "gt" and t.dtype == torch.uint8
            maps.append(t.detach().to(device=self.device, dtype=torch.uint8 if keep else torch.int32).contiguous().view(-1))
        if maps[0].numel() != maps[1].numel():
            raise ValueError(f"label_iou: pred holds {maps[0].numel()} pixels, gt {maps[1].numel()}")
        fresh = totals is None
        if fresh:
            totals = torch.empty(3, C_, dtype=torch.int64, device=self.device)
        elif not isinstance(totals, torch.Tensor) or totals.dtype != torch.int64 or tuple(totals.shape) != (3, C_) or \
                totals.device != maps[0].device or not totals.is_contiguous():
            raise ValueError(f"label_iou: totals must be what an earlier call with num_classes = {C_} returned")
        hip.label_iou_hist(maps[0], maps[1], C_, ignore_index, bool(reduce_zero_label), fresh, totals)
        return totals

    # ---- panoptic quality ----------------------------------------------------------------------------------------------
    def _pq_map(self, who: str, name: str, m, rgb: bool = False) -> torch.Tensor:
        """A flat map of a panoptic call on this engine's device: int32 (pixels,), or uint8 (pixels, 3) for an RGB id image.  A list holds
        one array per image and is laid back to back."""
        if isinstance(m, (list, tuple)) and m and all(isinstance(a, (torch.Tensor, np.ndarray)) for a in m):
            parts = [torch.as_tensor(a) for a in m]
            m = torch.cat([a.reshape(-1, 3) if rgb else a.reshape(-1) for a in parts])
        t = _integer_map(who, name, m, int32=not rgb)
        if rgb:
            if t.dtype != torch.uint8 or t.shape[-1] != 3:
                raise ValueError(f"{who}: with rgb=True {name} must be uint8 with a last axis of 3, got {t.dtype} {tuple(t.shape)}")
            return t.detach().to(device=self.device).contiguous().view(-1, 3)
        return t.detach().to(device=self.device, dtype=torch.int32).contiguous().view(-1)

    def panoptic_remap(self, raw, sizes, segments, *, rgb: bool = False) -> "PanopticGroundTruth":
        """A panoptic ground truth as cvlm_pan_pair_hist reads it (cvlm_pan_remap) -> PanopticGroundTruth: `gt`, the dense
        slot index of every pixel, `unknown` (B,), and the slot tables `gt_cat` / `gt_crowd` for panoptic_quality.  raw: the images' id
        maps back to back at the B sizes (h, w) of `sizes`, or a list of one array per image -- integers (the ids), or with rgb=True the
        uint8 (h, w, 3) pixels of COCO's panoptic PNGs (id = R + 256 G + 65536 B).  segments: per image its annotation's segments_info
        as (id, category, iscrowd) triples, in annotation order: slot i + 1 is the i-th.  Id 0 is void; an id the annotation does not
        list becomes void and is counted in `unknown`.  No synchronisation.  ValueError before anything is launched."""
        if not isinstance(rgb, (bool, np.bool_)):
            raise ValueError(f"panoptic_remap: rgb must be a bool, got {rgb!r}")
        sizes = _image_sizes(sizes, "panoptic_remap")
        B = len(sizes)
        keys, vals, offsets, gt_cat, gt_crowd = pq_segments_request(segments, B)
        t = self._pq_map("panoptic_remap", "raw", raw, bool(rgb))
        dims, pix_offsets, max_pixels = label_tables(sizes)
        if t.shape[0] != int(pix_offsets[-1]):
            raise ValueError(f"panoptic_remap: raw holds {t.shape[0]} pixels, sizes {int(pix_offsets[-1])}")
        up, i32 = partial(_upload, dev=self.device), partial(_empty, self.device)
        out = PanopticGroundTruth(gt=i32(t.shape[0]), unknown=i32(B), gt_cat=gt_cat, gt_crowd=gt_crowd,
                                  status=torch.zeros(1, dtype=torch.int32, device=self.device), sizes=sizes)
        hip.pan_remap(t, B, up(dims), up(pix_offsets), max_pixels, up(keys), up(vals), up(offsets), out.gt, out.unknown, out.status)
        return out

    def panoptic_quality(self, pred, pred_cat, gt, gt_cat, gt_crowd, sizes, *, num_classes: int, totals=None) -> "PanopticTotals":
        """Panoptic quality's sums of a predicted panoptic map against ground truth, on the device (cvlm_pan_pair_hist / match /
        accumulate) -> PanopticTotals, whose `counts` and `iou_sum` `segeval.pq_average` turns into PQ, SQ and RQ.  pred,
        gt: dense segment indices, 0 = void, back to back at the B sizes of `sizes` (or a list of one array per image) -- e.g.
        `LabelMaps.pq_inputs(classes)` and `panoptic_remap(...).gt`; pred_cat (B, S), gt_cat (B, G): a slot's category in [0,
        num_classes) or -1, slot 0 = -1; gt_crowd (B, G): iscrowd.  totals: the result of an earlier call, accumulated into -- a dataset's
        batches sum on the device, and `status` with them; None starts from zero.  The per-image tensors are the last call's.  One
        (B, G, S) int32 table is allocated per call.  No synchronisation.  ValueError (`pq_request`) before anything is launched."""
        maps = [self._pq_map("panoptic_quality", n, m) for n, m in (("pred", pred), ("gt", gt))]
        sizes, pred_cat, gt_cat, gt_crowd, G, S = pq_request(pred_cat, gt_cat, gt_crowd, sizes, num_classes=num_classes,
                                                             n_pred=maps[0].numel(), n_gt=maps[1].numel())
        C_ = int(num_classes)
        if totals is not None and not (isinstance(totals, PanopticTotals) and totals.num_classes == C_ and totals.counts.device == maps[0].device):
            raise ValueError(f"panoptic_quality: totals must be what an earlier call with num_classes = {C_} returned")
        B = len(sizes)
        dev = self.device
        up = lambda a: a if isinstance(a, torch.Tensor) else _upload(a, dev)
        pred_cat, gt_cat, gt_crowd = up(pred_cat).contiguous(), up(gt_cat).contiguous(), up(gt_crowd).contiguous()
        dims, pix_offsets, max_pixels = label_tables(sizes)
        i32, f64 = partial(_empty, dev), partial(_empty, dev, dtype=torch.float64)
        fresh = totals is None
        out = PanopticTotals(counts=i32(3, C_, dtype=torch.int64) if fresh else totals.counts, iou_sum=f64(C_) if fresh else totals.iou_sum,
                             status=torch.zeros(1, dtype=torch.int32, device=dev) if fresh else totals.status,
                             inter=i32(B, G, S), pred_match=i32(B, S), pred_iou=f64(B, S),
                             gt_match=i32(B, G), pred_area=i32(B, S), gt_area=i32(B, G), num_classes=C_)
        hip.pan_pair_hist(maps[0], maps[1], B, G, S, up(dims), up(pix_offsets), max_pixels, True, out.inter, out.status)
        hip.pan_match(out.inter, pred_cat, gt_cat, gt_crowd, C_, out.pred_match, out.pred_iou, out.gt_match, out.pred_area, out.gt_area)
        hip.pan_accumulate(pred_cat, gt_cat, out.pred_match, out.pred_iou, out.gt_match, C_, fresh, out.counts, out.iou_sum)
        return out

    def mask_rle_sized(self, sized: "SizedMasks") -> "MaskRle":
        """COCO run-length encoding of sized planes -> MaskRle whose `to_coco()` writes each plane's own "size": [h, w],
        what an evaluator holds against an annotation of the original image.  One cvlm_mask_rle_count_w call per run of consecutive
        planes of one size -- per image where the planes come from the engine --, one torch.cumsum, ONE read of the total (the call's
        only synchronisation), then one cvlm_mask_rle_emit_w call per run through the workspace "cls_rle", all on absolute offsets
        into one `counts`.  The status words of the runs are folded into one on the device."""
        sizes = _sized_arg("mask_rle_sized", "sized", sized).sizes
        P, dev = len(sizes), sized.bits.device
        i32 = partial(_empty, dev)
        _, host_off, _ = sized.tables()
        runs, a = [], 0                                               # (first plane, one past the last) of each run of equal sizes
        for p in range(1, P + 1):
            if p == P or sizes[p] != sizes[a]:
                runs.append((a, p))
                a = p
        n_runs = i32(P)
        rows = lambda a, b: sized.bits[int(host_off[a]):int(host_off[b])].view(b - a, -1)
        for a, b in runs:
            h, w = sizes[a]
            hip.mask_rle_count_w(rows(a, b), h, 32 * ((w + 31) // 32), w, n_runs[a:b])
        offsets = torch.zeros(P + 1, dtype=torch.int64, device=dev)
        torch.cumsum(n_runs, 0, dtype=torch.int64, out=offsets[1:])
        total = int(offsets[P].item())                               # the one synchronisation
        counts, status = i32(total), i32(len(runs))
        want = 0
        for a, b in runs:
            h, w = sizes[a]
            pitch = 32 * ((w + 31) // 32)
            want = max(want, _capped(hip.mask_rle_workspace_bytes(b - a, h, pitch), hip.mask_rle_workspace_bytes(1, h, pitch), RLE_WS_CAP))
        ws = self.ws.scratch("cls_rle", want)
        for i, (a, b) in enumerate(runs):
            h, w = sizes[a]
            hip.mask_rle_emit_w(rows(a, b), h, 32 * ((w + 31) // 32), w, offsets[a:b + 1], counts, status[i:i + 1], ws)
        same = all(s == sizes[0] for s in sizes)
        return MaskRle(counts=counts, offsets=offsets, n_runs=n_runs, size=sizes[0] if same else None,
                       status=torch.amax(status, 0, keepdim=True), sizes=sizes)

    # ---- COCO annotations on the device --------------------------------------------------------------------------------
    def rle_decode(self, rles, *, stats: bool = True) -> "SizedMasks":
        """COCO run-length annotations -> SizedMasks on this engine's device (cvlm_mask_rle_decode): ground truth in the
        format of the predictions, on which `mask_inter_sized`, `mask_rle_sized` and -- per image -- `mask_components`, `mask_holes` and
        `mask_morph` run.  rles: a list of {"size": [h, w], "counts": list | bytes | str}, checked by `rle_decode_request` on the host
        before anything is launched (ValueError) and uploaded once; or a MaskRle already on the device, e.g. `mask_rle_sized`'s: then
        nothing is copied to the host and nothing synchronises -- the kernel's own checks are the only ones, and `check()` of the
        result reports what they refused (a refused plane is zero).  stats=False: no `area` and no `box`.  The result has level 0:
        not a threshold.  The workspace is the grow-only "cls_rle", capped at RLE_WS_CAP (beyond it the entry walks the planes in
        rounds).  Launches on the caller's stream."""
        dev = self.device
        if isinstance(rles, MaskRle):
            P = int(rles.n_runs.shape[0])
            sizes = [tuple(rles.size_of(p)) for p in range(P)]
            if not 1 <= P <= 65535 or not rles.counts.is_cuda or rles.counts.dtype != torch.int32 or rles.counts.numel() < 1 or \
                    any(not 1 <= v <= SIZED_MAX_SIDE for s in sizes for v in s):
                raise ValueError("rle_decode: a MaskRle of 1 .. 65535 planes on the device, sides in [1, 16384]")
            counts, run_offsets = rles.counts.contiguous(), rles.offsets.contiguous()
        else:
            c, o, sizes = rle_decode_request(rles)
            counts, run_offsets = _upload(c, dev), _upload(o, dev)
        out, dims, max_pixels, ws = self._decoded(sizes, stats, hip.mask_rle_decode_workspace_bytes)
        hip.mask_rle_decode(counts, run_offsets, dims, out.offsets, max_pixels, out.bits, out.area, out.box, out.status, ws)
        return out

    def _decoded(self, sizes, stats: bool, workspace_bytes):
        """What the two decoders share behind their entries: the result's planes with their offsets uploaded, the planes' dims uploaded,
        the largest plane's pixel count and the workspace "cls_rle" by the entry's own size query, capped at RLE_WS_CAP."""
        out, dims, _ = SizedMasks.empty(sizes, self.device, level=0, stats=stats)
        max_pixels = max(h * w for h, w in sizes)
        one = workspace_bytes(1, max_pixels)
        return out, _upload(dims, self.device), max_pixels, self.ws.scratch("cls_rle", _capped(len(sizes) * one, one, RLE_WS_CAP))

    # ---- COCO polygon annotations on the device -------------------------------------------------------------------------
    def polygons_decode(self, anns, *, stats: bool = True) -> "SizedMasks":
        """COCO polygon annotations -> SizedMasks on this engine's device (cvlm_mask_poly_decode): what pycocotools'
        frPyObjects + merge + decode give for an iscrowd = 0 annotation, bit for bit, as ground truth in the format of the predictions
        -- `mask_inter_sized`, `mask_rle_sized` and ground_truth= of infer_classes / decode take it as it is; `SizedMasks.concat` joins it
        with `rle_decode`'s crowd regions.  anns: a list of {"size": [h, w], "polygons": [[x0, y0, x1, y1, ...], ...]}, one plane per
        entry, the union of its polygons; checked by `polygons_request` on the host before anything is launched (ValueError) and
        uploaded once per table.  stats=False: no `area` and no `box`.  The result has level 0: not a threshold; `check()` reports a
        plane the kernel refused.  The workspace is the grow-only "cls_rle", capped at RLE_WS_CAP (beyond it the entry walks the
        planes in rounds).  Launches on the caller's stream, without a synchronisation."""
        dev = self.device
        xy, po, pp, sizes = polygons_request(anns)
        out, dims, max_pixels, ws = self._decoded(sizes, stats, hip.mask_poly_decode_workspace_bytes)
        hip.mask_poly_decode(_upload(xy, dev), _upload(po, dev), _upload(pp, dev), dims, out.offsets, max_pixels, out.bits, out.area, out.box,
                             out.status, ws)
        return out

    def mask_inter_sized(self, a: "SizedMasks", b: "SizedMasks", *, pairs=None, a_image=None, b_image=None) -> "SizedOverlaps":
        """Intersections of pairs of sized planes -> SizedOverlaps (cvlm_mask_inter_sized): detections `a` against
        annotations `b` (they may be the same object).  Either pairs= -- (N, 2) (plane of a, plane of b) -- or a_image= and b_image=, one
        image id per plane of each: all (p, q) with a_image[p] == b_image[q], ordered by p, then q; `pairs_request` checks them on the
        host before anything is launched (ValueError).  Two planes of different sizes give inter = -1, as pycocotools' rleIou does.
        One upload of the pair table and of the two small size tables, one launch pair, two gathers of the areas; no workspace, no
        synchronisation: `SizedOverlaps.iou()` does the one read."""
        for name, s in (("a", a), ("b", b)):
            _sized_arg("mask_inter_sized", name, s, areas=True)
        table = pairs_request(a.sizes, b.sizes, pairs=pairs, a_image=a_image, b_image=b_image)
        dev = a.bits.device
        tab = table.to(torch.int32).contiguous() if isinstance(table, torch.Tensor) else _upload(table, dev)
        N = int(tab.shape[0])
        a_dims, _, a_words = a.tables()
        b_dims, _, b_words = (a_dims, None, a_words) if b is a else b.tables()
        a_dims = _upload(a_dims, dev)
        b_dims = a_dims if b is a else _upload(b_dims, dev)
        inter, status = _empty(dev, N), _empty(dev, 1)
        hip.mask_inter_sized(a.bits, a.offsets, a_dims, b.bits, b.offsets, b_dims, tab, max(a_words, b_words), inter, status)
        pick = lambda s, col: s.area.index_select(0, tab[:, col].long().clamp_(0, len(s.sizes) - 1))
        return SizedOverlaps(pairs=tab, inter=inter, area_a=pick(a, 0), area_b=pick(b, 1), status=status)


    # ---- Boundary IoU ---------------------------------------------------------------------------------------------------
    def mask_boundary_sized(self, sized: "SizedMasks", *, dilation_ratio=BOUNDARY_RATIO, radius=None) -> "SizedMasks":
        """The boundary of each sized plane -> SizedMasks of the same sizes, offsets and level (cvlm_mask_boundary_sized):
        boundary_iou_api's mask_to_boundary -- the mask without its erosion by a square of radius d, pixels outside the image read as
        clear, d = `boundary_radius` of the plane's own (h, w) or radius= --, at a cost that does not grow with d.  `boundary_request`
        checks the arguments on the host before anything is launched (ValueError).  `area` is the boundary's pixel count and `box` a
        clone of the input's (the box of a non-empty boundary is its mask's) when the input has them, both None when it has not;
        `status` is the kernel's.  The result feeds `mask_inter_sized`, `mask_rle_sized` and `SizedMasks.concat` as it is: the Boundary
        IoU of pairs is `mask_inter_sized(boundary(a), boundary(b), ...).iou()`.  One upload of the radius table and of the size
        table, a workspace as large as the planes from torch.empty, no synchronisation."""
        _sized_arg("mask_boundary_sized", "sized", sized)
        radii = boundary_request(sized.sizes, dilation_ratio=dilation_ratio, radius=radius)
        dev, i32 = sized.bits.device, partial(_empty, sized.bits.device)
        dims, _, max_words = sized.tables()
        stats = sized.area is not None
        out = SizedMasks(bits=torch.empty_like(sized.bits), offsets=sized.offsets, area=i32(len(sized.sizes)) if stats else None,
                         box=sized.box.clone() if stats else None, status=i32(1), sizes=[tuple(z) for z in sized.sizes], level=sized.level)
        hip.mask_boundary_sized(sized.bits, sized.offsets, _upload(dims, dev), _upload(radii, dev), max_words, torch.empty_like(sized.bits),
                                out.bits, out.area, out.status)
        return out

    # ---- Contours: COCO polygons out ---------------------------------------------------------------------------------------
    def mask_contours_sized(self, sized: "SizedMasks", *, connectivity=8) -> "MaskContours":
        """The crack contour of each sized plane -> MaskContours (cvlm_mask_contour_count / cvlm_mask_contour_emit), whose
        `to_coco()` is the polygon list of an iscrowd = 0 annotation and of the reference's GenericMask.  `contour_request` checks the
        arguments on the host before anything is launched (ValueError).  The count, one torch.cumsum, ONE read of n_vertices (the
        call's only synchronisation), then the host cuts the planes into rounds whose workspace stays within RLE_WS_CAP -- a plane
        that needs more on its own is a round of its own -- and one emit call per round goes through the grow-only workspace
        "cls_rle".  The status words are folded into one on the device.  Launches on the caller's stream."""
        _sized_arg("mask_contours_sized", "sized", sized)
        sizes, connectivity = contour_request(sized.sizes, connectivity=connectivity)
        P, dev = len(sizes), sized.bits.device
        i32 = partial(_empty, dev)
        dims, _, max_words = sized_tables(sizes)
        dims = _upload(dims, dev)
        n_vertices, count_status = i32(P), i32(1)
        hip.mask_contour_count(sized.bits, sized.offsets, dims, connectivity, max_words, n_vertices, count_status)
        offsets = torch.zeros(P + 1, dtype=torch.int64, device=dev)
        torch.cumsum(n_vertices, 0, dtype=torch.int64, out=offsets[1:])
        counted = n_vertices.cpu().numpy()                           # the one synchronisation
        total = int(counted.astype(np.int64).sum())
        rounds = contour_rounds(counted, max_words, RLE_WS_CAP, hip.mask_contour_workspace_bytes)
        xy, ring_start = i32(total, 2, dtype=torch.int16), i32(total, dtype=torch.uint8)
        n_rings, status = i32(P, 2), i32(len(rounds))
        ws = self.ws.scratch("cls_rle", max(r[3] for r in rounds))
        for i, (a, b, rv, need) in enumerate(rounds):
            hip.mask_contour_emit(sized.bits, sized.offsets[a:b + 1], dims[a:b], connectivity, max_words, offsets[a:b + 1], rv, xy, ring_start,
                                  n_rings[a:b], status[i:i + 1], ws[:need])
        return MaskContours(xy=xy, ring_start=ring_start, vertex_offsets=offsets, n_vertices=n_vertices, n_rings=n_rings, sizes=sizes,
                            connectivity=connectivity, status=torch.maximum(torch.amax(status, 0, keepdim=True), count_status))

    # ---- Simplified contour rings: Douglas-Peucker polygons out ---------------------------------------------------------------
    def simplify_contours(self, contours: "MaskContours", *, tolerance=1.0) -> "MaskPolygons":
        """The rings of a MaskContours simplified on the device -> MaskPolygons (cvlm_contour_simplify_mark / cvlm_contour_simplify_emit,
        DESIGN.md §34): Ramer-Douglas-Peucker on every closed ring, in exact integers, at `tolerance` pixels (a multiple of 0.25, one for
        all planes or one per plane; 0 returns the rings as they are).  `simplify_request` checks the arguments on the host before
        anything is launched (ValueError).  The mark runs in rounds whose workspace stays within RLE_WS_CAP through the grow-only
        workspace "cls_rle" -- the whole input as one round when it fits, which needs no look at the counts; otherwise the host reads
        the input's vertex counts and cuts the planes as `contour_rounds` does --, then one torch.cumsum of the kept counts, ONE read
        of their total (the only synchronisation of a call that fits one round), the outputs, the emit.  The status words are folded
        into one on the device together with the input's: a plane the contour call refused comes out empty and sets it.  Launches
        on the caller's stream."""
        if not isinstance(contours, MaskContours) or not contours.xy.is_cuda:
            raise ValueError(f"simplify_contours: contours must be a MaskContours on the device, got {type(contours).__name__}")
        T = simplify_request(contours, tolerance=tolerance)
        P, dev, total = len(contours.sizes), contours.xy.device, int(contours.xy.shape[0])
        i32 = partial(_empty, dev)
        need = lambda planes, vertices, _=0: hip.contour_simplify_workspace_bytes(planes, vertices)
        rounds = [(0, P, total, need(P, total))]
        if rounds[0][3] > RLE_WS_CAP and P > 1:
            rounds = contour_rounds(contours.n_vertices.cpu().numpy(), 0, RLE_WS_CAP, need)
        T_dev = _upload(T, dev)
        keep, n_kept, n_rings, status = i32(total, dtype=torch.uint8), i32(P), i32(P, 2), i32(len(rounds) + 1)
        ws = self.ws.scratch("cls_rle", max(r[3] for r in rounds))
        for i, (a, b, rv, nbytes) in enumerate(rounds):
            hip.contour_simplify_mark(contours.xy, contours.ring_start, contours.vertex_offsets[a:b + 1], T_dev[a:b], rv, keep, n_kept[a:b],
                                      n_rings[a:b], status[i:i + 1], ws[:nbytes])
        offsets = torch.zeros(P + 1, dtype=torch.int64, device=dev)
        torch.cumsum(n_kept, 0, dtype=torch.int64, out=offsets[1:])
        total_out = int(offsets[P].item())                           # the one read of the counts
        xy, ring_start = i32(total_out, 2, dtype=torch.int16), i32(total_out, dtype=torch.uint8)
        hip.contour_simplify_emit(contours.xy, contours.ring_start, contours.vertex_offsets, keep, offsets, xy, ring_start, status[-1:])
        n_dropped = (contours.n_rings.sum(1) - n_rings.sum(1)).clamp_(min=0).to(torch.int32)
        return MaskPolygons(xy=xy, ring_start=ring_start, vertex_offsets=offsets, n_vertices=n_kept, n_rings=n_rings, n_dropped=n_dropped,
                            sizes=[tuple(z) for z in contours.sizes], tolerance=T.astype(np.float64) / 4.0,
                            status=torch.maximum(torch.amax(status, 0, keepdim=True), contours.status.reshape(-1)[:1].to(torch.int32)))

    # ---- Distance maps and surface distances ----------------------------------------------------------------------------------
    @staticmethod
    def _distance(bits, offsets, sizes, reach, out_d2, ws, status) -> None:
        """One cvlm_mask_distance_sized call on planes that lie back to back, into out_d2 in label_tables' layout."""
        dev = bits.device
        dims, _, max_words = sized_tables(sizes)
        _, pix, _ = label_tables(sizes)
        hip.mask_distance_sized(bits, offsets, _upload(dims, dev), _upload(reach, dev), max_words, _upload(pix, dev), ws, out_d2, status)

    def mask_distance_sized(self, sized: "SizedMasks", *, reach=None) -> "MaskDistances":
        """The squared Euclidean distance map of each sized plane -> MaskDistances (cvlm_mask_distance_sized): for every
        pixel the exact squared distance to the plane's nearest set pixel, DISTANCE_FAR where none is within reach.  reach: None for an
        unlimited search; an int, or one per plane, in [1, 23170] keeps D2 <= reach^2 exact, makes everything else far and bounds every
        pixel's work by O(reach).  `distance_request` checks the arguments on the host before anything is launched (ValueError).
        Memory: 4 bytes per pixel of result and 2 bytes per pixel of the grow-only workspace "cls_rle".  One upload of the three small
        tables, three launches on the caller's stream, no synchronisation."""
        _sized_arg("mask_distance_sized", "sized", sized)
        sizes, reaches = distance_request(sized.sizes, reach=reach)
        dev, i32 = sized.bits.device, partial(_empty, sized.bits.device)
        _, pix, _ = label_tables(sizes)
        n_pix = int(pix[-1])
        out = MaskDistances(d2=i32(n_pix), pix_offsets=_upload(pix, dev), sizes=sizes, reach=reaches, status=i32(1))
        ws = self.ws.scratch("cls_rle", (2 * n_pix + 15) // 16 * 16)
        self._distance(sized.bits, sized.offsets, sizes, reaches, out.d2, ws, out.status)
        return out

    @staticmethod
    def _take_planes(sized: "SizedMasks", planes: list):
        """(bits, offsets, sizes) of the named planes lying back to back: the input's own tensors where all are named in order, a
        gather of their byte ranges otherwise (the ranges come from the sizes: no read of the device)."""
        if planes == list(range(len(sized.sizes))):
            return sized.bits, sized.offsets, list(sized.sizes)
        _, off, _ = sized.tables()
        sizes = [sized.sizes[p] for p in planes]
        bits = torch.cat([sized.bits[int(off[p]):int(off[p + 1])] for p in planes])
        return bits, _upload(sized_tables(sizes)[1], bits.device), sizes

    def mask_surface_distances(self, a: "SizedMasks", b: "SizedMasks", *, pairs=None, tolerance=SURFACE_RATIO, surface="boundary",
                               reach=None) -> "SurfaceTotals":
        """How far the contours of pairs of planes lie apart -> SurfaceTotals (cvlm_mask_distance_sized + cvlm_mask_surface_totals, DESIGN.md
        §27), from which `surfeval.surface_metrics` gives the Hausdorff distance, the average symmetric surface distance, the normalised
        surface Dice and the boundary F-measure.  a: predictions, b: annotations (they may be the same object); pairs: (N, 2) (plane of
        a, plane of b), None for plane p against plane p; tolerance: one or up to 8, ints in pixels or ratios of each pair's diagonal
        (`surface_tolerance`; 0.008 is the published boundary F-measure's); reach: None -- unlimited, what Hausdorff and ASSD need -- or
        "tolerance", which bounds every search by the pair's largest radius and leaves NSD and F exact; `surface_request` checks all of
        it on the host before anything is launched (ValueError).
        surface="boundary": the surface of a mask is `mask_boundary_sized(radius=1)` -- a set pixel with a clear or outside pixel among
        its eight neighbours; this is §25's boundary, NOT the published measure's own seg2bmap --; surface=None takes the planes as given:
        edge maps, which are contours already.
        The call never holds all maps: the host cuts the pairs into rounds whose maps stay within RLE_WS_CAP (6 bytes per pixel of the
        planes a round names; one pair at least), and per round and direction runs the distance entry on the planes the round names and
        then the totals entry, through the grow-only workspace "cls_rle", on the caller's stream.  A plane named by many pairs is
        transformed once per round it appears in.  No synchronisation: `SurfaceTotals.to_host()` does the one read."""
        for name, s in (("a", a), ("b", b)):
            _sized_arg("mask_surface_distances", name, s)
        if surface is not None and not (isinstance(surface, str) and surface == "boundary"):
            raise ValueError(f"mask_surface_distances: surface must be 'boundary' or None, got {surface!r}")
        req = surface_request(a.sizes, b.sizes, pairs=pairs, tolerance=tolerance, reach=reach)
        dev = a.bits.device
        N, T = req.radii.shape
        rounds = surface_rounds(req.pairs, req.a_sizes, req.b_sizes, RLE_WS_CAP)
        if surface is not None:
            sa = self.mask_boundary_sized(a, radius=1)
            sb = sa if b is a else self.mask_boundary_sized(b, radius=1)
        else:
            sa, sb = a, b
        i32 = partial(_empty, dev)
        table = lambda: dict(n=i32(N), far=i32(N), within=i32(N, T), max_d2=i32(N), sum_d2=i32(N, dtype=torch.int64),
                             sum_d=i32(N, dtype=torch.float64))
        out = SurfaceTotals(pairs=_upload(req.pairs, dev), radii=_upload(req.radii, dev), ab=table(), ba=table(), status=None)
        status = i32(len(rounds), 4)
        r16 = lambda v: (v + 15) // 16 * 16
        need = lambda px, n: r16(4 * px) + r16(2 * px) + hip.mask_surface_workspace_bytes(n)
        pixels = lambda sizes, planes: sum(sizes[p][0] * sizes[p][1] for p in planes)
        ws = self.ws.scratch("cls_rle", max(need(max(pixels(req.a_sizes, ua), pixels(req.b_sizes, ub)), i1 - i0) for i0, i1, ua, ub, _ in rounds))
        dims_of = {id(s): _upload(s.tables()[0], dev) for s in (sa, sb)}
        words_of = {id(s): s.tables()[2] for s in (sa, sb)}
        for r, (i0, i1, ua, ub, _) in enumerate(rounds):
            # direction 0, "ab": the pixels of a's surfaces against the maps of the b planes of the round; direction 1 the reverse
            for way, (pix_src, map_src, named, reaches, col, tab) in enumerate(((sa, sb, ub, req.reach_b, 1, out.ab),
                                                                               (sb, sa, ua, req.reach_a, 0, out.ba))):
                bits, offsets, sizes = self._take_planes(map_src, named)
                _, pix, _ = label_tables(sizes)
                px = int(pix[-1])
                d2 = ws[:4 * px].view(torch.int32)
                f = ws[r16(4 * px):r16(4 * px) + r16(2 * px)]
                part = ws[r16(4 * px) + r16(2 * px):need(px, i1 - i0)]
                self._distance(bits, offsets, sizes, reaches[named], d2, f, status[r, 2 * way:2 * way + 1])
                local = np.searchsorted(named, req.pairs[i0:i1, col]).astype(np.int32)
                pr = np.ascontiguousarray(np.stack([req.pairs[i0:i1, 1 - col], local], axis=1))
                hip.mask_surface_totals(pix_src.bits, pix_src.offsets, dims_of[id(pix_src)], d2, _upload(pix, dev),
                                        _upload(sized_tables(sizes)[0], dev), _upload(pr, dev), out.radii[i0:i1],
                                        words_of[id(pix_src)], part, tab["n"][i0:i1], tab["far"][i0:i1], tab["within"][i0:i1],
                                        tab["max_d2"][i0:i1], tab["sum_d2"][i0:i1], tab["sum_d"][i0:i1], status[r, 2 * way + 1:2 * way + 2])
        out.status = torch.amax(status.reshape(-1), 0, keepdim=True)
        if surface is not None:                                       # the boundaries' own refusals are the call's as well
            for s in {id(sa): sa, id(sb): sb}.values():
                out.status = torch.maximum(out.status, s.status.reshape(-1)[:1].ne(0).to(torch.int32))
        return out

    # ---- Thinning: skeletons, thin edges, clDice -------------------------------------------------------------------------------
    def _thin(self, bits, offsets, sizes, limits, mode, steps, out_bits, area, box, iters, done, status) -> None:
        """One cvlm_mask_thin_sized call on planes that lie back to back, through the grow-only workspace "cls_rle"."""
        dev = bits.device
        dims, _, max_words = sized_tables(sizes)
        ws = self.ws.scratch("cls_rle", hip.mask_thin_workspace_bytes(int(bits.numel()), len(sizes), steps))
        hip.mask_thin_sized(bits, offsets, _upload(dims, dev), _upload(limits, dev), max_words, mode, steps, ws, out_bits, area, box, iters, done,
                            status)

    def mask_thin_sized(self, sized: "SizedMasks", *, max_iter=None, path="auto", steps=64) -> "MaskThin":
        """Each sized plane reduced to its centre lines -> MaskThin (cvlm_mask_thin_sized): Guo & Hall's thinning -- MATLAB's
        bwmorph(X, 'thin', n), scikit-image's thin(X, max_num_iter) --, to the fixed point or for max_iter iterations.  The result is a
        subset of the input with as many 8-connected components; `MaskThin.masks` is a SizedMasks of the same sizes, offsets and level
        with an area and a box of its own, and feeds `mask_inter_sized`, `mask_rle_sized`, `mask_distance_sized` and their kin as it is.
        `thin_request` checks the arguments on the host before anything is launched (ValueError).
        path="auto": a plane that fits the resident kernel's LDS (`hip.mask_thin_resident`: 1024 x 1024 does) is thinned to its end by
        one workgroup; where every plane is resident the call is one upload of the two small tables and one entry call, without a
        synchronisation.  The other planes -- every plane under path="steps" -- are stepped in rounds of `steps` iterations: each round is
        followed by ONE read of done (and status), then the next round runs on the planes that are not yet done, gathered back to back,
        their output as the input and their max_iter less the iterations spent -- exact, because the state of the rule is the bits alone.
        Workspace: the grow-only "cls_rle", as many bytes as the planes of a round plus 4 * steps per plane."""
        _sized_arg("mask_thin_sized", "sized", sized)
        sizes, limits, mode, steps = thin_request(sized.sizes, max_iter=max_iter, path=path, steps=steps)
        P, dev = len(sizes), sized.bits.device
        i32 = partial(_empty, dev)
        out = MaskThin(masks=SizedMasks(bits=torch.empty_like(sized.bits), offsets=sized.offsets, area=i32(P), box=i32(P, 4), status=i32(1),
                                        sizes=sizes, level=sized.level), iters=i32(P), done=i32(P), status=None)
        out.status = out.masks.status
        fits = hip.load().cvlm_mask_thin_resident                      # host arithmetic, no launch
        left = [p for p, (h, w) in enumerate(sizes) if mode == 1 or not fits(h, w)]
        self._thin(sized.bits, sized.offsets, sizes, limits, mode, steps if left else 0, out.masks.bits, out.masks.area, out.masks.box,
                   out.iters, out.done, out.status)
        _, off, _ = sized_tables(sizes)
        spent = 0
        while left:
            flags = torch.cat([out.done, out.status]).cpu().numpy()   # the round's one read
            spent += steps
            left = [p for p in left if flags[p] == 0]
            if flags[P] != 0 or not left:                             # a refused plane is never done: check() reports it
                break
            idx = torch.tensor(left, dtype=torch.int64, device=dev)
            part = [sizes[p] for p in left]
            bits = torch.cat([out.masks.bits[int(off[p]):int(off[p + 1])] for p in left])
            rest = np.where(limits[left] == 0, 0, limits[left] - spent).astype(np.int32)      # > 0 where limited: the plane is not done
            r_bits, r_area, r_box, r_iters, r_done, r_status = torch.empty_like(bits), i32(len(left)), i32(len(left), 4), i32(len(left)), \
                i32(len(left)), i32(1)
            self._thin(bits, _upload(sized_tables(part)[1], dev), part, rest, mode, steps, r_bits, r_area, r_box, r_iters, r_done, r_status)
            at = 0
            for p in left:
                n = int(off[p + 1] - off[p])
                out.masks.bits[int(off[p]):int(off[p + 1])] = r_bits[at:at + n]
                at += n
            out.masks.area[idx] = r_area
            out.masks.box[idx] = r_box
            out.iters[idx] += r_iters
            out.done[idx] = r_done
            out.status |= r_status
        return out

    def mask_cldice(self, a: "SizedMasks", b: "SizedMasks", *, pairs=None, a_image=None, b_image=None) -> "ClDiceTotals":
        """The counts of centre-line Dice (clDice, Shit et al., CVPR 2021) of pairs of sized planes -> ClDiceTotals, from
        which `surfeval.cldice` gives Tprec = |S_A & B| / |S_A|, Tsens = |S_B & A| / |S_B| and their harmonic mean: the overlap that
        notices a missing limb.  a: predictions, b: annotations (they may be the same object); pairs= or a_image= / b_image= as
        `mask_inter_sized` takes them, on the host (`pairs_request` checks them before anything is launched, ValueError); none of the
        three: plane p against plane p.  Both sides are thinned once, to their fixed points (`mask_thin_sized`), then two `mask_inter_sized`
        calls count the skeletons inside the other side's masks, the second with the pair columns swapped.  No synchronisation beyond
        `mask_thin_sized`'s: none where every plane is resident."""
        for name, s in (("a", a), ("b", b)):
            _sized_arg("mask_cldice", name, s, areas=True)
        if isinstance(pairs, torch.Tensor) and pairs.is_cuda:         # the second count swaps the columns on the host
            raise ValueError("mask_cldice: pairs must be (N, 2) ints on the host")
        if pairs is None and a_image is None and b_image is None:
            pairs = _plane_by_plane("mask_cldice", len(a.sizes), len(b.sizes), "pairs= or image ids")
        table = pairs_request(a.sizes, b.sizes, pairs=pairs, a_image=a_image, b_image=b_image, who="mask_cldice")
        ta = self.mask_thin_sized(a)
        tb = ta if b is a else self.mask_thin_sized(b)
        ab = self.mask_inter_sized(ta.masks, b, pairs=table)
        ba = self.mask_inter_sized(tb.masks, a, pairs=np.ascontiguousarray(table[:, ::-1]))
        status = torch.maximum(torch.maximum(ta.status, tb.status), torch.maximum(ab.status, ba.status)).ne(0).to(torch.int32)
        return ClDiceTotals(pairs=ab.pairs, skel_a=ab.area_a, skel_a_in_b=ab.inter, skel_b=ba.area_a, skel_b_in_a=ba.inter, status=status)

    # ---- Instances: the regions of sized planes as planes of their own ---------------------------------------------------------
    def mask_regions_sized(self, sized: "SizedMasks", *, regions: int = 8, min_area: int = 0, connectivity: int = 8) -> "MaskRegions":
        """Each sized plane split into its connected regions -> MaskRegions (cvlm_mask_regions_sized): the number of
        regions of at least max(min_area, 1) pixels, the `regions` largest with their boxes and seeds, and each of those as a sized
        plane of its own, of the source plane's size -- `MaskRegions.masks` feeds `mask_rle_sized`, `mask_contours_sized`, `coco_match`
        and their kin as it is, `MaskRegions.compact()` drops the empty slots.  `regions_request` checks the arguments on the host
        before anything is launched (ValueError).  One upload of the two small tables and one entry call on the caller's stream,
        without a synchronisation; the grow-only workspace "cls_comp" holds every plane in flight up to COMPONENTS_WS_CAP (and never
        less than the largest plane), beyond it the entry walks the planes in rounds."""
        _sized_arg("mask_regions_sized", "sized", sized)
        sizes, M, min_area, connectivity = regions_request(sized.sizes, regions=regions, min_area=min_area, connectivity=connectivity)
        P, dev = len(sizes), sized.bits.device
        dims, _, max_words = sized_tables(sizes)
        slots = [z for z in sizes for _ in range(M)]
        i32 = partial(_empty, dev)
        n_regions, table, status = i32(P), i32(P, M, 6), i32(1)
        n_bytes = int(sized.bits.numel())
        out_bits = i32(M * n_bytes, dtype=torch.uint8)
        want = _capped(hip.mask_regions_workspace_bytes(n_bytes, P, max_words), hip.mask_regions_workspace_bytes(4 * max_words, 1, max_words),
                       COMPONENTS_WS_CAP)
        hip.mask_regions_sized(sized.bits, sized.offsets, _upload(dims, dev), max_words, connectivity, min_area,
                               self.ws.scratch("cls_comp", want), n_regions, table, out_bits, status)
        masks = SizedMasks(bits=out_bits, offsets=_upload(sized_tables(slots)[1], dev), area=table[..., 0].reshape(P * M),
                           box=table[..., 1:5].reshape(P * M, 4), status=status, sizes=slots, level=sized.level)
        return MaskRegions(n_regions=n_regions, table=table, masks=masks, M=M)

    # ---- Mask NMS across the hypotheses of each image ------------------------------------------------------------------------
    def mask_nms_sized(self, instances: "SizedMasks", *, scores, image, category=None, iou=0.5, measure: str = "iou", method: str = "greedy",
                       sigma: float = 2.0) -> "MaskNms":
        """The duplicate instances of each image dropped or decayed -> MaskNms (cvlm_mask_nms_inter + cvlm_mask_nms).
        instances: a SizedMasks on this engine's device with areas and boxes, e.g. `MaskRegions.compact()`'s.  scores: one per instance,
        a float32 tensor on the device taken as it is (NaN ranks last), or a host sequence.  category: None (class-agnostic), or one int
        per instance -- an integer tensor on the device, e.g. `RegionClasses.pred`, or a host sequence -- and only instances of one
        category suppress each other.  image and the other arguments are `nms_request`'s, which checks them on the host before anything
        is launched (ValueError).  One upload of the three tables and the sizes, the two entry calls on the caller's stream, no workspace, no
        synchronisation: `MaskNms.select(instances)` does the one read.  No instance: empty tensors, nothing launched."""
        _sized_arg("mask_nms_sized", "instances", instances, areas=True, boxes=True, empty=True)
        dev, Q = instances.bits.device, len(instances.sizes)
        i32 = partial(_empty, dev)
        if Q == 0:
            if len(image) != 0 or len(scores) != 0 or (category is not None and len(category) != 0):
                raise ValueError("mask_nms_sized: scores, image and category must hold one value per instance, 0 of them")
            return MaskNms(keep=i32(0, dtype=torch.uint8), by=i32(0), decay=i32(0, dtype=torch.float32), order=i32(0), n_keep=i32(0), inter=i32(0),
                           status=torch.zeros(2, dtype=torch.int32, device=dev))
        req = nms_request(instances.sizes, image=image, iou=iou, measure=measure, method=method, sigma=sigma)

        def column(name, v, dtype, kinds):
            if isinstance(v, torch.Tensor) and v.is_cuda:
                ok = v.dtype == torch.float32 if dtype == torch.float32 else v.dtype in (torch.int32, torch.int64, torch.int16, torch.uint8)
                if not ok or tuple(v.shape) != (Q,):
                    raise ValueError(f"mask_nms_sized: {name} on the device must be a {'float32' if dtype == torch.float32 else 'integer'} tensor ({Q},)")
                return v.detach().to(dtype).contiguous()
            try:
                arr = np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v)
            except Exception as err:
                raise ValueError(f"mask_nms_sized: {name} must hold one number per instance") from err
            if arr.shape != (Q,) or arr.dtype.kind not in kinds:
                raise ValueError(f"mask_nms_sized: {name} must hold one number per instance, {Q} of them")
            return _upload(arr.astype(np.float32 if dtype == torch.float32 else np.int32), dev)

        score = column("scores", scores, torch.float32, "iuf")
        cat = None if category is None else column("category", category, torch.int32, "iu")
        G = len(req.keys)
        dims = np.ascontiguousarray(instances.tables()[0])
        tables = np.concatenate([req.pair_offsets.view(np.uint8), req.group_offsets.view(np.uint8), req.member.view(np.uint8),
                                 dims.reshape(-1).view(np.uint8)])
        tables = _upload(tables, dev)                                 # the one upload: the int64 table first, so every view is aligned
        pair_offsets = tables[:8 * (G + 1)].view(torch.int64)
        group_offsets = tables[8 * (G + 1):12 * (G + 1)].view(torch.int32)
        member = tables[12 * (G + 1):12 * (G + 1) + 4 * Q].view(torch.int32)
        dims = tables[12 * (G + 1) + 4 * Q:].view(torch.int32).view(Q, 2)
        status = i32(2)
        out = MaskNms(keep=i32(Q, dtype=torch.uint8), by=i32(Q), decay=i32(Q, dtype=torch.float32), order=i32(Q), n_keep=i32(G),
                      inter=i32(req.n_pairs), status=status, request=req)
        hip.mask_nms_inter(instances.bits, instances.offsets, dims, instances.area.contiguous(), instances.box.contiguous(), group_offsets,
                           member, pair_offsets, out.inter, status[0:1])
        hip.mask_nms(group_offsets, member, pair_offsets, out.inter, instances.area.contiguous(), score, cat, req.measure, req.method,
                     req.thr, req.sigma, out.order, out.keep, out.by, out.decay, out.n_keep, status[1:2])
        return out

    # ---- Rendering: overlays, outlines and label colour maps ------------------------------------------------------------------
    def render(self, images: "SizedImages", layers, *, host: bool = False) -> "Rendered":
        """The layers painted over the images -> Rendered, a new SizedImages with the kernel's status (cvlm_render).
        images: a SizedImages on the device (`sized_images`); layers: one sequence per image of what `fill`, `heat` and `classes` built,
        applied in order.  `render_request` checks everything on the host before anything is launched (ValueError).  One upload of the
        tables, one entry call on the caller's stream, no workspace, no synchronisation; layers whose sources are different tensors
        cost one torch.cat of those per kind.  No layer for any image: nothing is launched and the result is a clone.  The pad bytes
        behind an image of the result are not written.  host=True: images and sources on the HOST, through the sequential host entry
        (cvlm_debug_render_host) -- for tests and for looking at a result where there is no device, never taken silently."""
        if not isinstance(images, SizedImages) or not isinstance(images.data, torch.Tensor) or images.data.is_cuda == bool(host):
            raise ValueError("render: images must be a SizedImages on the device (host=True: on the host)")
        dev = images.data.device
        req = render_request(images.sizes, layers, device=dev)
        sizes = [tuple(z) for z in images.sizes]
        if req.L == 0:
            return Rendered(data=images.data.clone(), offsets=images.offsets, dims=images.dims, sizes=sizes,
                            status=torch.zeros(1, dtype=torch.int32, device=dev))
        B, L, T = len(sizes), req.L, int(req.alpha.shape[0])
        tables = np.concatenate([req.layers.reshape(-1).view(np.uint8), req.layer_offsets.view(np.uint8), req.alpha.view(np.uint8),
                                 req.rgb.reshape(-1)])
        tables = _upload(tables, dev)                                 # the one upload: the int64 table first, so every view is aligned
        at = np.cumsum([0, 32 * L, 4 * (B + 1), 4 * T, 3 * T])
        rows = tables[at[0]:at[1]].view(torch.int64).view(L, 4)
        layer_offsets = tables[at[1]:at[2]].view(torch.int32)
        alpha = tables[at[2]:at[3]].view(torch.float32)
        rgb = tables[at[3]:at[4]].view(T, 3)

        def buffer(kind):
            parts = req.sources[kind]
            if not parts:
                return None
            t = parts[0] if len(parts) == 1 else torch.cat(parts)
            return t.clone() if t.data_ptr() % 4 else t               # the kernel reads bits and labels as 32-bit words

        out = Rendered(data=torch.empty_like(images.data), offsets=images.offsets, dims=images.dims, sizes=sizes,
                       status=torch.empty(1, dtype=torch.int32, device=dev))
        _, _, max_pixels = image_tables(sizes)
        hip.render(images.data, images.offsets, images.dims, max_pixels, layer_offsets, rows, buffer(0), buffer(1), buffer(2), rgb, alpha,
                   out.data, out.status, host=bool(host))
        return out

    def render_overlay(self, images: "SizedImages", sized: "SizedMasks", *, image_of, colors=(0, 255, 0), alpha=0.5, outline=None,
                       outline_color=(255, 255, 255), host: bool = False) -> "Rendered":
        """demo.py's picture without its text (save_array_as_image, lines 51-56): every plane of `sized` painted over image image_of[p]
        in its colour at `alpha` -- colors: one colour for all planes or one per plane, in the images' channel order --, the planes of
        an image in their order.  outline=r: the boundary of radius r of every plane (`mask_boundary_sized`) painted afterwards in
        outline_color at alpha 1.  `render_overlay(images, pack_masks_sized(logits, sizes, level=1), image_of=range(B))` is the demo's
        `overlay[data_array > 0] = (0, 255, 0)` blended half and half.  host=True: `render`'s, without outline=."""
        if not isinstance(images, SizedImages) or not isinstance(sized, SizedMasks):
            raise ValueError("render_overlay: images must be a SizedImages and sized a SizedMasks")
        B, P = len(images.sizes), len(sized.sizes)
        if not _is_seq(image_of) or len(image_of) != P:
            raise ValueError(f"render_overlay: image_of must hold one image index per plane, {P} of them")
        image_of = [_render_index("render_overlay", "an image index", b, B) for b in image_of]
        cols = np.asarray(colors)
        if cols.ndim == 1:
            cols = np.broadcast_to(cols, (P,) + cols.shape)
        if cols.shape != (P, 3):
            raise ValueError(f"render_overlay: colors must be one colour or hold one per plane, {P} of them")
        layers = [[] for _ in range(B)]
        for p, b in enumerate(image_of):
            layers[b].append(fill(sized, p, color=cols[p], alpha=alpha))
        if outline is not None:
            if host or not images.data.is_cuda:
                raise ValueError("render_overlay: outline= needs images and planes on the device")
            render_request(images.sizes, layers, device=images.data.device, who="render_overlay")    # everything, before the first launch
            _render_colors("render_overlay", "outline_color", [outline_color] if np.ndim(outline_color) == 1 else outline_color, 1)
            edges = self.mask_boundary_sized(sized, radius=outline)
            for p, b in enumerate(image_of):
                layers[b].append(fill(edges, p, color=outline_color, alpha=1.0))
        return self.render(images, layers, host=host)

    # ---- COCO matching on the device ---------------------------------------------------------------------------------------
    def coco_match(self, dets: Optional["SizedMasks"], gts: Optional["SizedMasks"], *, scores, det_image, gt_image, det_category=None,
                   gt_category=None, iscrowd=None, gt_area=None, iou_thrs=None, area_rngs=None, max_det: int = 100,
                   boundary=None) -> "CocoMatches":
        """Detections against annotations as COCOeval.evaluateImg matches them -> CocoMatches (cvlm_coco_match), for every
        (image, category) group, area range and IoU threshold at once; `cocoeval.accumulate` / `summarize` turn it into AP and AR.  dets
        / gts: SizedMasks on this engine's device with areas, e.g. `sized` of infer_classes / decode and `rle_decode` /
        `polygons_decode` of the annotations; None for a side without planes.  scores: one per plane of dets -- a float32 tensor on the
        device, taken as it is (NaN ranks last), or a host sequence (NaN: ValueError).  The other arguments are `match_request`'s, which
        checks all of them on the host before anything is launched (ValueError).  Then: `mask_inter_sized(pairs=...)` for the groups'
        pair blocks (skipped when no group has both sides), gathers of the areas and scores into table order, one cvlm_coco_match call.
        No workspace, no synchronisation: `CocoMatches.to_host()` does the one read.
        boundary=ratio (None: exactly the launches and allocations above): the matching compares min(mask IoU, boundary
        IoU) with the thresholds, as boundary_iou_api's COCOeval with iouType = "boundary" does -- `accumulate` / `summarize` over the
        result are Boundary AP and AR.  ratio is `boundary_request`'s dilation ratio, 0.02 in the published evaluators.  Added, in this
        order: `mask_boundary_sized` of dets and of gts, a second `mask_inter_sized(pairs=...)` on the boundaries (kept as
        `boundary_overlaps`), the gathers of the boundaries' areas, and cvlm_coco_match_boundary in place of cvlm_coco_match.  The area
        ranges keep using the masks' areas and gt_area."""
        for name, s in (("dets", dets), ("gts", gts)):
            _sized_arg("coco_match", name, s, areas=True, optional=True)
        d_sizes, g_sizes = ([] if s is None else s.sizes for s in (dets, gts))
        on_device = isinstance(scores, torch.Tensor) and scores.is_cuda
        if on_device and (scores.dtype != torch.float32 or tuple(scores.shape) != (len(d_sizes),)):
            raise ValueError(f"coco_match: scores on the device must be a float32 tensor ({len(d_sizes)},)")
        req = match_request(d_sizes, g_sizes, det_image=det_image, gt_image=gt_image, det_category=det_category, gt_category=gt_category,
                            iscrowd=iscrowd, gt_area=gt_area, scores=None if on_device else scores, iou_thrs=iou_thrs, area_rngs=area_rngs,
                            max_det=max_det)
        if not on_device and req.scores is None:
            raise ValueError("coco_match: scores must hold one number per detection")
        if boundary is not None:
            for s in (dets, gts):
                if s is not None:
                    boundary_request(s.sizes, dilation_ratio=boundary, who="coco_match")
        dev = self.device
        up, i32 = partial(_upload, dev=dev), partial(_empty, dev)
        ND, NG = int(req.det_perm.size), int(req.gt_perm.size)
        A, T = int(req.area_rngs.shape[0]), int(req.iou_thrs.size)
        overlaps = self.mask_inter_sized(dets, gts, pairs=req.pairs) if req.pairs.shape[0] else None
        inter = overlaps.inter if overlaps is not None else i32(0)
        if ND:
            det_perm = up(req.det_perm)
            det_area = dets.area.index_select(0, det_perm)
            score = scores.detach().index_select(0, det_perm) if on_device else up(req.scores)
        else:
            det_area, score = i32(0), torch.empty(0, dtype=torch.float32, device=dev)
        if NG:
            g_area = gts.area.index_select(0, up(req.gt_perm))
            range_area = g_area.to(torch.float64) if req.range_area is None else up(req.range_area)
        else:
            g_area, range_area = i32(0), torch.empty(0, dtype=torch.float64, device=dev)
        u8 = partial(_empty, dev, dtype=torch.uint8)
        out = CocoMatches(dt_order=i32(ND), dt_match=i32(A, T, ND), dt_ignore=u8(A, T, ND), gt_match=i32(A, T, NG), gt_ignore=u8(A, NG), score=score,
                          status=i32(1), overlaps=overlaps, request=req)
        if boundary is None:
            hip.coco_match(up(req.det_offsets), up(req.gt_offsets), up(req.pair_offsets), inter, det_area.contiguous(), score.contiguous(),
                           g_area.contiguous(), range_area.contiguous(), up(req.crowd), up(req.iou_thrs), up(req.area_rngs), req.max_det,
                           out.dt_order, out.dt_match, out.dt_ignore, out.gt_match, out.gt_ignore, out.status)
            return out
        none = i32(0)
        det_b = None if dets is None else self.mask_boundary_sized(dets, dilation_ratio=boundary)
        gt_b = None if gts is None else det_b if gts is dets else self.mask_boundary_sized(gts, dilation_ratio=boundary)
        out.boundary_overlaps = self.mask_inter_sized(det_b, gt_b, pairs=req.pairs) if req.pairs.shape[0] else None
        inter_b = out.boundary_overlaps.inter if out.boundary_overlaps is not None else none
        det_area_b = det_b.area.index_select(0, det_perm) if ND else none
        gt_area_b = gt_b.area.index_select(0, up(req.gt_perm)) if NG else none
        hip.coco_match_boundary(up(req.det_offsets), up(req.gt_offsets), up(req.pair_offsets), inter, det_area.contiguous(),
                                score.contiguous(), g_area.contiguous(), range_area.contiguous(), up(req.crowd), up(req.iou_thrs),
                                up(req.area_rngs), req.max_det, inter_b, det_area_b.contiguous(), gt_area_b.contiguous(), out.dt_order,
                                out.dt_match, out.dt_ignore, out.gt_match, out.gt_ignore, out.status)
        return out


COMPONENT_FIELDS = ("n_comp", "comps", "n_kept", "kept_bits", "kept_area", "kept_box")


class MaskPost:
    """What one Cascade.infer_classes / decode call does for its arguments masks= .. ground_truth=, for n images with K hypotheses each
    and masks `side` pixels wide: the one plan both entry points run, so that they cannot differ in it.  The constructor is the eight
    request checks, in the order of the arguments, on the host: it raises ValueError under the caller's name `who` and allocates and
    launches nothing.  Then, on the stream the entry point decodes on: `allocate_planes` and `allocate` make the result tensors, each
    chunk of prompts p0 <= p < p1 gets its planes from `chunk_planes` and, once the decoder has written them, `chunk`; `finish` runs
    what follows the last chunk.  The results are attributes under their ClassHypotheses field names (FIELDS), None where not asked
    for; `fields()` is the constructor's keywords, `outputs()` / `inputs()` the tensors another stream must be told of.
    masks= / overlaps= (`compact_request`): "bits" or "both" add `mask_bits`, `area` and `box` -- cvlm_mask_pack on each
    chunk's full-resolution planes --, overlaps=True `inter`, one cvlm_mask_overlap launch behind the last chunk.  "bits" returns no
    `masks` and no `edges`: the planes of a chunk live in a workspace buffer of class_chunk() planes, from which `_alpha` reads them,
    the edge maps are not resized, and no (B, K, S, S) tensor exists; the decoder's launches are those of the default call, so every
    other field keeps its bits.  The default, masks="logits", overlaps=False, makes exactly the launches and allocations of a call
    without this family.
    components= / min_area= / connectivity= (`components_request`; they need masks="bits" or "both"): components=M adds
    `n_comp` and `comps`, the connected regions of each packed mask and its M largest; min_area >= 1 adds `n_kept`, `kept_bits`,
    `kept_area` and `kept_box`, the mask without its regions below min_area pixels -- cvlm_mask_components on each chunk's rows of
    `mask_bits`.  A descriptor, not a rule: nothing is ranked or chosen between hypotheses.
    holes= / fill_holes= (`holes_request`; they need masks="bits" or "both" and share connectivity=): holes=M adds
    `n_holes` and `holes`, the holes of each packed mask and its M largest; fill_holes >= 1 adds `n_filled`, `filled_bits` and
    `filled_area`, the mask with its holes of fewer than fill_holes pixels set -- cvlm_mask_holes on each chunk's rows of `mask_bits`,
    behind cvlm_mask_components.  Independent of components=: `kept_*` stay functions of `mask_bits`; SAM's order, fill then
    despeckle, is mask_components(mask_holes(bits, ...).filled_bits, ...).
    band=r (`morph_request`; needs masks="bits" or "both"): adds `band_bits` and `band_area`, the edge band of each
    packed mask -- dilation & ~erosion by the (2 r + 1)^2 square, r = 2 the band the reference trains its edge head against -- by
    cvlm_mask_morph on each chunk's rows of `mask_bits`, right behind the packs, into the result's own tensors: no workspace.  With
    overlaps=True also `band_inter`, the bands' pairwise intersections, one more cvlm_mask_overlap launch behind the last chunk:
    boundary agreement of two hypotheses is band_inter / (band_area_a + band_area_b - band_inter), and the caller divides.
    Independent of components= and holes=.
    edge_threshold=t (`edge_request`; 0 < t < 1, needs masks="bits" or "both"): adds `edge_bits` and `edge_area`, the
    edge head's probability map of each hypothesis as bits -- one cvlm_edge_pack call per chunk, right behind the band, that resizes
    the decoder's low-resolution edge map, compares `> t` and packs, into the result's own tensors: no workspace, and no
    full-resolution edge map even with masks="both", so edge_bits is the same function of the decoder's output in both modes (it may
    differ from `edges > t` only where |edges - t| <= 2^-21).  With band=r also `edge_band`, the edge pixels on each mask's band;
    with overlaps=True also `edge_inter`, one more cvlm_mask_overlap launch behind the last chunk.  The decoder's launches are those
    of the call without it.  Nothing is chosen here and there is no default threshold: the reference trains and evaluates the soft
    map.
    rle="mask" / "kept" / "filled" (`rle_request`; needs masks="bits" or "both", "kept" needs min_area >= 1, "filled"
    fill_holes >= 1): adds `rle`, the COCO run-length encoding of mask_bits, kept_bits or filled_bits of all n * K hypotheses --
    `mask_rle`, once, behind the last chunk where cvlm_mask_overlap runs: two count launches, a cumsum, one read of the total (a
    synchronisation of the host with the stream) and the emit's launches.  An interchange format for pycocotools, the COCO / LVIS
    evaluators and the reference's GenericMask, not a compression: see DESIGN.md §18 for sizes.
    sizes= / sized_level= (`sized_request`; they need masks="bits" or "both"): sizes holds one (h, w) per image, the
    size of the ORIGINAL image the evaluation compares at; adds `sized`, a SizedMasks with the K masks of image b at (h_b, w_b) -- the
    bits of the reference's uint8 mask (sigmoid, cv2.resize to (h, w), * 255) >= sized_level, with areas and boxes in the image's
    coordinates -- by one cvlm_mask_pack_sized call per chunk on the chunk's full-resolution planes, right behind cvlm_mask_pack, into
    the result's own tensors: no workspace, and with masks="bits" still no f32 plane in the result.  The two tables of the planes are
    built on the host and uploaded once, before the first chunk.  rle="sized" (needs sizes=) encodes those planes, `mask_rle_sized`,
    behind the last chunk: `rle.to_coco()` then carries "size": [h, w] of each image, which an evaluator can hold against an
    annotation.
    ground_truth=(gt, gt_image) (`ground_truth_request`; needs sizes=): gt is a SizedMasks of annotations -- `rle_decode`
    of their COCO RLEs -- and gt_image[q] the image of the call annotation q belongs to, whose size it must have; adds `gt_overlaps`,
    a SizedOverlaps with the intersection of every hypothesis's sized plane with every annotation of its own image -- pairs
    (b * K + k, q) ordered by the plane, then q --, by one cvlm_mask_inter_sized call behind the last chunk; `gt_overlaps.iou(iscrowd)`
    is the COCO IoU.  Nothing is matched or chosen.
    label_maps=True / label_weights= / overlap_threshold= (`labels_request`; needs sizes=): adds `label_maps`, a
    LabelMaps with one hypothesis per pixel of each image at its own size -- Mask2Former's panoptic_inference at the level sized_level,
    the weights (B, K) being the caller's scores.  cvlm_label_init with the other allocations, the weights uploaded before the first
    chunk, one cvlm_label_accumulate per chunk right behind cvlm_mask_pack_sized on the chunk's planes while they sit in the workspace,
    cvlm_label_finish behind the last chunk: about 8 bytes per image pixel, no (B, K, S, S) tensor, no synchronisation.
    Each option is independent of the others: without it the call makes exactly the launches, allocations and synchronisations it
    makes with the others alone, and every other field keeps its bits."""
    FIELDS = ("masks", "edges", "mask_bits", "area", "box", "inter") + COMPONENT_FIELDS + HOLE_FIELDS + BAND_FIELDS + EDGE_FIELDS + \
        ("rle", "sized", "gt_overlaps", "label_maps")

    def __init__(self, *, who: str, n: int, K: int, side: int, masks="logits", overlaps=False, components=None, min_area=0, connectivity=8,
                 holes=None, fill_holes=0, band=None, edge_threshold=None, rle=None, sizes=None, sized_level=128, ground_truth=None,
                 label_maps=False, label_weights=None, overlap_threshold=0.8):
        self.n, self.K, self.side = n, K, side
        self.want_logits, self.want_bits, self.want_inter = compact_request(masks=masks, overlaps=overlaps, n=n, K=K, who=who)
        self.want_comps, self.comps_m, self.min_area, self.connectivity = components_request(
            components=components, min_area=min_area, connectivity=connectivity, masks=masks, side=side, who=who)
        self.want_holes, self.holes_m, self.fill_below, _ = holes_request(holes=holes, fill_holes=fill_holes, connectivity=connectivity,
                                                                          masks=masks, side=side, who=who)
        self.want_band, self.band_radius, self.want_band_inter = morph_request(band=band, masks=masks, overlaps=overlaps, side=side, who=who)
        self.want_edges, self.edge_t, self.want_edge_band, self.want_edge_inter = edge_request(
            edge_threshold=edge_threshold, masks=masks, overlaps=overlaps, band=band, side=side, who=who)
        self.rle_source = rle_request(rle=rle, masks=masks, min_area=min_area, fill_holes=fill_holes, side=side, who=who)
        sreq = sized_request(sizes=sizes, sized_level=sized_level, n=n, masks=masks, rle=rle, who=who)
        self.sizes, self.sized_level = (None, None) if sreq is None else sreq
        greq = ground_truth_request(ground_truth, sreq, n, who=who)
        self.gt, self.gt_image = (None, None) if greq is None else greq
        self.labels_req = labels_request(label_maps=label_maps, sizes=sizes, weights=label_weights, level=sized_level,
                                         overlap_threshold=overlap_threshold, n=n, K=K, masks=masks, who=who)
        self.label_weights_in = label_weights if isinstance(label_weights, torch.Tensor) and label_weights.is_cuda else None
        for f in self.FIELDS:
            setattr(self, f, None)

    def allocate_planes(self, engine) -> None:
        """`masks` and `edges`, the first of the result's allocations, for the call of `engine` (a Cascade) that runs this plan."""
        self.engine = engine
        if self.want_logits:
            self.masks = torch.empty(self.n, self.K, self.side, self.side, device=engine.device)
            self.edges = torch.empty(self.n, self.K, self.side, self.side, device=engine.device)

    def allocate(self, chunk: int) -> None:
        """Every other result tensor, in the order of the arguments, then `sized` with its two tables uploaded; `chunk` prompts at most
        will come per `chunk` call."""
        eng, n, K, nbytes = self.engine, self.n, self.K, self.side * self.side // 8
        u8 = lambda *shape: torch.empty(*shape, dtype=torch.uint8, device=eng.device)
        i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=eng.device)
        if self.want_bits:
            self.mask_bits, self.area, self.box = u8(n, K, nbytes), i32(n, K), i32(n, K, 4)
            self.inter = i32(n, K, K) if self.want_inter else None
        if self.want_comps:
            self.n_comp, self.comps, self.n_kept, self.kept_bits, self.kept_area, self.kept_box = \
                eng._component_outputs((n, K), nbytes, self.comps_m, self.min_area)
        if self.want_holes:
            self.n_holes, self.holes, self.n_filled, self.filled_bits, self.filled_area = eng._hole_outputs((n, K), nbytes, self.holes_m, self.fill_below)
        if self.want_band:
            self.band_bits, self.band_area = u8(n, K, nbytes), i32(n, K)
            self.band_inter = i32(n, K, K) if self.want_band_inter else None
        if self.want_edges:
            self.edge_bits, self.edge_area = u8(n, K, nbytes), i32(n, K)
            self.edge_band = i32(n, K) if self.want_edge_band else None
            self.edge_inter = i32(n, K, K) if self.want_edge_inter else None
        if self.sizes is not None:
            self.sized, self.sized_dims, self.sized_max_words = eng._sized_outputs(self.sizes, self.sized_level, K, -(-n * K // chunk))
        if self.labels_req is not None:
            self.label_maps, self.label_weights, self.label_max_pixels = eng._label_outputs(self.sizes, K, *self.labels_req)

    def chunk_planes(self, p0: int, p1: int):
        """Where the full-resolution planes of the prompts p0 <= p < p1 go: the result's tensors, or with masks="bits" the workspace
        buffer "cls_planes" of at most class_chunk() planes and no edge map -> (mask planes, edge planes or None)."""
        S = self.side
        if self.masks is not None:
            return self.masks.view(-1, S, S)[p0:p1], self.edges.view(-1, S, S)[p0:p1]
        return self.engine.ws.f32("cls_planes", p1 - p0, S, S), None

    def chunk(self, planes: torch.Tensor, p0: int, p1: int, call: int) -> None:
        """The packed outputs of the prompts p0 <= p < p1, the call-th chunk, from their full-resolution `planes`, into rows p0 .. p1 - 1
        of the result's tensors: cvlm_mask_pack, cvlm_mask_pack_sized, then on the packed rows cvlm_mask_morph (band only),
        cvlm_edge_pack, cvlm_mask_components and cvlm_mask_holes, each where asked for."""
        eng, S = self.engine, self.side
        rows = lambda t, own: _rows(t, own, p0, p1)
        bits = rows(self.mask_bits, 1)
        if self.want_bits:
            hip.mask_pack(planes, bits, rows(self.area, 0), rows(self.box, 1))
        if self.sized is not None:
            eng._pack_sized(planes, self.sized, self.sized_dims, self.sized_max_words, p0, p1, call)
        if self.label_maps is not None:
            eng._label_accumulate(planes, self.label_maps, self.label_weights, self.label_max_pixels, p0, p1)
        if self.want_band:
            hip.mask_morph(bits, S, S, self.band_radius, band_bits=rows(self.band_bits, 1), band_area=rows(self.band_area, 0))
        if self.want_edges:
            # the chunk's low-resolution edge map where MaskDecoder left it, workspace buffer "low_edge", (p1 - p0) x 4G x 4G: the full-
            # resolution edge map is not formed; with band=, edge_band against the chunk's rows of band_bits
            L = 4 * eng.g.grid
            low = eng.decoder.ws.f32("low_edge", p1 - p0, L * L).view(p1 - p0, L, L)
            on_band = self.edge_band is not None
            hip.edge_pack(low, S, S, self.edge_t, rows(self.edge_bits, 1), rows(self.edge_area, 0),
                          rows(self.band_bits, 1) if on_band else None, rows(self.edge_band, 0))
        if self.want_comps:
            eng._components(bits, S, S, self.connectivity, self.min_area,
                            [rows(getattr(self, f), own) for f, own in zip(COMPONENT_FIELDS, (0, 2, 0, 1, 0, 1))])
        if self.want_holes:
            eng._holes(bits, S, S, self.connectivity, self.fill_below, [rows(getattr(self, f), own) for f, own in zip(HOLE_FIELDS, (0, 2, 0, 1, 0))])

    def finish(self) -> None:
        """Behind the last chunk: the cvlm_mask_overlap launches of `inter`, `band_inter` and `edge_inter`, `rle` -- `mask_rle` of the
        planes `rle_request` named, all n * K at once, or `mask_rle_sized` of the sized planes, with its one host read --, then
        `gt_overlaps`, `mask_inter_sized` of the sized planes with the annotations of each plane's own image."""
        eng = self.engine
        if self.want_inter:
            hip.mask_overlap(self.mask_bits, self.inter)
        if self.want_band_inter:
            hip.mask_overlap(self.band_bits, self.band_inter)
        if self.want_edge_inter:
            hip.mask_overlap(self.edge_bits, self.edge_inter)
        if self.rle_source == RLE_SIZED:
            self.rle = eng.mask_rle_sized(self.sized)
        elif self.rle_source is not None:
            planes = getattr(self, self.rle_source)
            self.rle = eng.mask_rle(planes.view(-1, planes.shape[-1]), self.side, self.side)
        if self.gt is not None:
            self.gt_overlaps = eng.mask_inter_sized(self.sized, self.gt, a_image=[b for b in range(self.n) for _ in range(self.K)],
                                                    b_image=self.gt_image)
        if self.label_maps is not None:
            eng._label_finish(self.label_maps, self.label_max_pixels)

    def outputs(self) -> tuple:
        """Every tensor of the result but `masks` and `edges`, in the order of FIELDS: what the caller's stream must wait for."""
        out = [getattr(self, f) for f in self.FIELDS[2:-4]]
        if self.rle is not None:
            out += [self.rle.counts, self.rle.offsets, self.rle.n_runs, self.rle.status]
        if self.sized is not None:
            out += [self.sized.bits, self.sized.offsets, self.sized.area, self.sized.box, self.sized.status]
        if self.gt_overlaps is not None:
            o = self.gt_overlaps
            out += [o.pairs, o.inter, o.area_a, o.area_b, o.status]
        if self.label_maps is not None:
            m = self.label_maps
            out += [m.score, m.winner, m.segment, m.areas, m.segment_id, m.n_segments, m.status, m.dims, m.pix_offsets]
        return tuple(t for t in out if t is not None)

    def inputs(self) -> tuple:
        """The caller's tensors this plan reads on the decoding stream: the ground truth's and label weights given on the device."""
        ins = () if self.gt is None else (self.gt.bits, self.gt.offsets, self.gt.area)
        return ins if self.label_weights_in is None else ins + (self.label_weights_in,)

    def fields(self) -> dict:
        """The results as keywords of ClassHypotheses(...)."""
        return {f: getattr(self, f) for f in self.FIELDS}
