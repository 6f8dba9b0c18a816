"""ctypes binding of libcvlm_hip.so (include/cvlm.h) -- the only way compute happens in this package.

There is no CPU fallback: if the shared library is missing or a launch fails, a RuntimeError is
raised.  torch is used for device memory and streams only (tensors' ``data_ptr()`` are handed to the
C ABI together with the current HIP stream).
"""
from __future__ import annotations

import ctypes as C
import functools
import os
from typing import Optional, Tuple

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libcvlm_hip.so")

ACT_NONE, ACT_GELU, ACT_QUICKGELU, ACT_RELU, ACT_ABS_POST = 0, 1, 2, 3, 4

# The C ABI of include/cvlm.h, one line per function: "<return>:<parameters>", one letter per type -- i int / int32_t, l int64_t, f float,
# p a data pointer, G / A / I a pointer to GemmArgs / AttnArgs / GemmPlanInfo, z const char* -- and a final s for `void* stream`, which
# `_call` supplies.  tests/test_host_cpu.py holds every line against the header's prototype.
_SIGNATURES = {
    "cvlm_abi_version": "i:", "cvlm_target_arch": "z:",
    "cvlm_gemm": "i:Gs", "cvlm_gemm_workspace_bytes": "l:", "cvlm_debug_gemm_plan": "i:GiiI",
    "cvlm_layernorm": "i:plpipppfipppiis",
    "cvlm_add_rows": "i:ppifpppiis",
    "cvlm_ln_stats_merge": "i:pliifpps",
    "cvlm_row_stats_split": "i:pfpppliiils",
    "cvlm_row_stats_split_mx": "i:pfplplplpliiils",
    "cvlm_split_f32": "i:pppls",
    "cvlm_patchify": "i:pipiiiiippis",
    "cvlm_im2col3x3": "i:piiiipps",
    "cvlm_reinterpret_transpose": "i:piiifpps",
    "cvlm_attention": "i:As", "cvlm_attention_workspace_bytes": "l:A",
    "cvlm_small_attention": "i:plplplpliiiiis",
    "cvlm_small_attention_h2": "i:plplplplppliiiiis",
    "cvlm_dense_pe": "i:piips",
    "cvlm_mask_head": "i:pppiiips",
    "cvlm_mask_head_edge": "i:pppiiipps",
    "cvlm_mask_head_multi": "i:pppiiiipps",
    "cvlm_bilinear": "i:piiipiiis",
    "cvlm_clip_assemble": "i:ppppiiiips",
    "cvlm_overwrite_rows": "i:piiiiips",
    "cvlm_gather_rows": "i:piiipips",
    "cvlm_gather_rows_h2": "i:ppfiiipips",
    "cvlm_clip_head": "i:ppfiiipppps",
    "cvlm_topk_select": "i:piiipippps",
    "cvlm_text_assemble": "i:ppippipiiiips",
    "cvlm_clip_head_wide_workspace_bytes": "l:ii",
    "cvlm_clip_head_wide": "i:ppfiiipppppls",
    "cvlm_topk_select_wide": "i:piiipippps",
    "cvlm_expand_blocks": "i:piilpppppps",
    "cvlm_normalize_add": "i:ppiips",
    "cvlm_resample_u8": "i:piiiippiiips",
    "cvlm_u8_to_tensor": "i:piiiiiiiippps",
    "cvlm_mask_to_u8": "i:piiiiips",
    "cvlm_mask_joint_hist": "i:ppiiipps",
    "cvlm_mask_pack": "i:pilippps",
    "cvlm_mask_overlap": "i:piilps",
    "cvlm_mask_components_workspace_bytes": "l:iii",
    "cvlm_mask_components": "i:piiiiiiplpppppps",
    "cvlm_debug_mask_components_host": "i:piiiiiipppppp",
    "cvlm_mask_holes_workspace_bytes": "l:iii",
    "cvlm_mask_holes": "i:piiiiiiplppppps",
    "cvlm_debug_mask_holes_host": "i:piiiiiippppp",
    "cvlm_mask_morph": "i:piiiipppppps",
    "cvlm_debug_mask_morph_host": "i:piiiipppppp",
    "cvlm_edge_pack": "i:piiiiifpppps",
    "cvlm_debug_edge_pack_host": "i:piiiiifpppp",
    "cvlm_debug_edge_pack_staged": "i:iiii",
    "cvlm_mask_rle_workspace_bytes": "l:iii",
    "cvlm_mask_rle_count": "i:piiips",
    "cvlm_mask_rle_emit": "i:piiipplppls",
    "cvlm_debug_mask_rle_host": "i:piiippplp",
    "cvlm_mask_rle_count_w": "i:piiiips",
    "cvlm_mask_rle_emit_w": "i:piiiipplppls",
    "cvlm_debug_mask_rle_host_w": "i:piiiippplp",
    "cvlm_mask_pack_sized": "i:piiippipllppps",
    "cvlm_debug_mask_pack_sized_host": "i:piiippipllppp",
    "cvlm_mask_rle_decode_workspace_bytes": "l:il",
    "cvlm_mask_rle_decode": "i:plpppilplppppls",
    "cvlm_debug_mask_rle_decode_host": "i:plpppilplppp",
    "cvlm_mask_poly_decode_workspace_bytes": "l:il",
    "cvlm_mask_poly_decode": "i:plppppiilplppppls",
    "cvlm_debug_mask_poly_decode_host": "i:plppppiilplppp",
    "cvlm_mask_inter_sized": "i:plppiplppipilpps",
    "cvlm_debug_mask_inter_sized_host": "i:plppiplppipilpp",
    "cvlm_coco_match": "i:pppiplppipppipipiipppppps",
    "cvlm_debug_coco_match_host": "i:pppiplppipppipipiipppppp",
    "cvlm_mask_boundary_sized": "i:plpppilpppps",
    "cvlm_debug_mask_boundary_sized_host": "i:plpppilpppp",
    "cvlm_coco_match_boundary": "i:pppiplppipppipipiippppppppps",
    "cvlm_debug_coco_match_boundary_host": "i:pppiplppipppipipiippppppppp",
    "cvlm_mask_contour_workspace_bytes": "l:ill",
    "cvlm_mask_contour_count": "i:plppiilpps",
    "cvlm_mask_contour_emit": "i:plppiilplppplppls",
    "cvlm_debug_mask_contour_host": "i:plppiippppplp",
    "cvlm_contour_simplify_workspace_bytes": "l:il",
    "cvlm_contour_simplify_mark": "i:ppplpilpppppls",
    "cvlm_contour_simplify_emit": "i:ppplpippplps",
    "cvlm_debug_contour_simplify_host": "i:ppplpipppppplp",
    "cvlm_mask_distance_workspace_bytes": "l:il",
    "cvlm_mask_distance_sized": "i:plpppilplplpps",
    "cvlm_debug_mask_distance_sized_host": "i:plpppilplplpp",
    "cvlm_mask_surface_workspace_bytes": "l:l",
    "cvlm_mask_surface_totals": "i:plppipplpiplpilplppppppps",
    "cvlm_debug_mask_surface_totals_host": "i:plppipplpiplpilplppppppp",
    "cvlm_mask_thin_workspace_bytes": "l:lii",
    "cvlm_mask_thin_resident": "i:ii",
    "cvlm_mask_thin_sized": "i:plpppiliiplpppppps",
    "cvlm_debug_mask_thin_sized_host": "i:plpppiliiplpppppp",
    "cvlm_mask_regions_workspace_bytes": "l:lil",
    "cvlm_mask_regions_sized": "i:plppiliiiplpppps",
    "cvlm_debug_mask_regions_sized_host": "i:plppiliiipppp",
    "cvlm_region_alpha": "i:plppipiippps",
    "cvlm_debug_region_alpha_host": "i:plppipiippp",
    "cvlm_mask_nms_inter": "i:plppppipppilpps",
    "cvlm_debug_mask_nms_inter_host": "i:plppppipppilpp",
    "cvlm_mask_nms": "i:pppiplpppiiippppppps",
    "cvlm_debug_mask_nms_host": "i:pppiplpppiiippppppp",
    "cvlm_render": "i:plppilppiplplplppipps",
    "cvlm_debug_render_host": "i:plppilppiplplplppipp",
    "cvlm_label_init": "i:ppplppiipps",
    "cvlm_label_accumulate": "i:piiiiiipppipppllpps",
    "cvlm_label_finish": "i:iipppppllpppps",
    "cvlm_label_lookup": "i:piippllpipps",
    "cvlm_label_iou_hist": "i:ppiliiiips",
    "cvlm_debug_label_init_host": "i:ppplppiipp",
    "cvlm_debug_label_accumulate_host": "i:piiiiiipppipppllpp",
    "cvlm_debug_label_finish_host": "i:iipppppllpppp",
    "cvlm_debug_label_lookup_host": "i:piippllpipp",
    "cvlm_debug_label_iou_hist_host": "i:ppiliiiip",
    "cvlm_pan_remap": "i:piippllppplppps",
    "cvlm_pan_pair_hist": "i:ppiiippllipps",
    "cvlm_pan_match": "i:piiipppippppps",
    "cvlm_pan_accumulate": "i:iiipppppiipps",
    "cvlm_debug_pan_lds_cells": "i:",
    "cvlm_debug_pan_remap_host": "i:piippllppplppp",
    "cvlm_debug_pan_pair_hist_host": "i:ppiiippllipp",
    "cvlm_debug_pan_match_host": "i:piiipppippppp",
    "cvlm_debug_pan_accumulate_host": "i:iiipppppiipp",
    "cvlm_mask_wfm": "i:ppiiipppps",
    "cvlm_prob_quantise": "i:piiippps",
    "cvlm_prob_moments": "i:ppiiipppps",
    "cvlm_prob_wfm": "i:ppiiipppps",
    "cvlm_topk_accumulate": "i:ppiipps",
}
EXPORTS = list(_SIGNATURES)
ABI_VERSION = 12


class GemmArgs(C.Structure):
    _fields_ = [
        ("a_hi", C.c_void_p), ("a_lo", C.c_void_p), ("lda", C.c_int64), ("stride_a", C.c_int64),
        ("w_hi", C.c_void_p), ("w_lo", C.c_void_p), ("ldw", C.c_int64), ("stride_w", C.c_int64),
        ("bias", C.c_void_p),
        ("residual", C.c_void_p), ("ldr", C.c_int64), ("stride_r", C.c_int64),
        ("out_f32", C.c_void_p), ("ldo", C.c_int64), ("stride_o", C.c_int64),
        ("out_hi", C.c_void_p), ("out_lo", C.c_void_p), ("ldoh", C.c_int64), ("stride_oh", C.c_int64),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("batch", C.c_int32),
        ("alpha", C.c_float), ("act", C.c_int32), ("split", C.c_int32),
        ("ps_h", C.c_int32), ("ps_w", C.c_int32), ("ps_c2", C.c_int32),
        ("hm_S", C.c_int32), ("hm_H", C.c_int32), ("hm_hd", C.c_int32),
        ("out_scale", C.c_float), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
        ("ln_stats", C.c_void_p), ("ln_colsum", C.c_void_p), ("ln_eps", C.c_float), ("ln_D", C.c_int32),
        ("res_hi", C.c_void_p), ("res_lo", C.c_void_p), ("ldrh", C.c_int64), ("res_scale", C.c_float),
        ("row_stats", C.c_void_p),
        ("conv_h", C.c_int32), ("conv_w", C.c_int32), ("conv_c", C.c_int32),
        ("w_il", C.c_void_p), ("ldw_il", C.c_int64),
        ("a_il", C.c_int32), ("out_il", C.c_int32), ("res_il", C.c_int32),
        ("a_mx", C.c_int32), ("out_mx", C.c_int32), ("res_mx", C.c_int32),
        ("a_mxs", C.c_void_p), ("lda_s", C.c_int64),
        ("w_mx", C.c_void_p), ("ldw_mx", C.c_int64), ("w_mxs", C.c_void_p), ("ldw_s", C.c_int64),
        ("out_mxs", C.c_void_p), ("ldo_s", C.c_int64), ("ldol", C.c_int64), ("ldrl", C.c_int64),
        ("hm_nolo", C.c_int32),
    ]


class GemmLaunchInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n0", "N", "nbx", "nby", "grid_x", "grid_y", "block", "lds_bytes", "group_m", "tail_rem",
                                         "tail_split", "total_blocks", "sk_parts", "uses_workspace")] + [("kernel", C.c_char * 128)]


class GemmPlanInfo(C.Structure):
    """cvlm_gemm_plan_info (include/cvlm.h): what cvlm_debug_gemm_plan fills."""
    _fields_ = [("launches", C.c_int32), ("launch", GemmLaunchInfo * 2)]


class AttnArgs(C.Structure):
    _fields_ = [
        ("qkv_hi", C.c_void_p), ("qkv_lo", C.c_void_p), ("pad_hi", C.c_void_p), ("pad_lo", C.c_void_p),
        ("relh_hi", C.c_void_p), ("relh_lo", C.c_void_p), ("relw_hi", C.c_void_p), ("relw_lo", C.c_void_p),
        ("out_hi", C.c_void_p), ("out_lo", C.c_void_p),
        ("B", C.c_int32), ("S", C.c_int32), ("heads", C.c_int32), ("hd", C.c_int32),
        ("mode", C.c_int32), ("grid", C.c_int32), ("window", C.c_int32), ("causal", C.c_int32),
        ("split_qk", C.c_int32), ("split_pv", C.c_int32), ("scale", C.c_float), ("qkv_layout", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("q_rows", C.c_int32),
    ]


_CTYPES = {"i": C.c_int32, "l": C.c_int64, "f": C.c_float, "p": C.c_void_p, "s": C.c_void_p, "z": C.c_char_p,
           "G": C.POINTER(GemmArgs), "A": C.POINTER(AttnArgs), "I": C.POINTER(GemmPlanInfo)}
ABI = {name: (_CTYPES[sig[0]], [_CTYPES[c] for c in sig[2:]]) for name, sig in _SIGNATURES.items()}    # name -> (restype, argtypes)
_STREAMED = frozenset(name for name, sig in _SIGNATURES.items() if sig.endswith("s"))

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load the shared library (once).  Raises RuntimeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("CVLM_PROBE_LIB") or LIB_PATH              # CVLM_PROBE_LIB: probe builds of the same ABI (tools/)
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the HIP kernels are the only compute path of this package. "
            "Build them with `python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950).")
    lib = C.CDLL(path)
    for name, (restype, argtypes) in ABI.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.cvlm_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{path}: ABI {lib.cvlm_abi_version()}, this binding needs {ABI_VERSION}: rebuild the library")
    _lib = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed with code {rc}")


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _pn(t: Optional[torch.Tensor]) -> Optional[int]:
    """`_p`, and NULL for an empty tensor too: the entries refuse a pointer that comes with a count of 0."""
    return t.data_ptr() if t is not None and t.numel() else None


def _workspace_bytes(symbol: str, *sizes) -> int:
    """The bytes of workspace the host arithmetic `symbol` of an entry gives for these sizes."""
    n = int(getattr(load(), symbol)(*(int(v) for v in sizes)))
    if n < 0:
        raise RuntimeError(f"{symbol}{tuple(int(v) for v in sizes)}: sizes outside the entry's bounds (code {n})")
    return n


def _planes(x: Optional["H2"]) -> Tuple[Optional[int], Optional[int]]:
    return (None, None) if x is None else (x.hi.data_ptr(), x.lo.data_ptr())


def _stream() -> Optional[int]:
    return torch.cuda.current_stream().cuda_stream or None


def _call(name: str, *args) -> None:
    """One call of the entry `name` with plain Python values (ints, floats, None for NULL, a struct for a struct pointer: `ABI` holds
    the C types); the current stream is appended where the entry takes one.  Raises on a non-zero return code."""
    fn = getattr(load(), name)
    _check(fn(*args, _stream()) if name in _STREAMED else fn(*args), name)


def _on_current_device(t: torch.Tensor) -> None:
    """Kernels launch on the CURRENT device's stream: a tensor living elsewhere would fault or silently go over xGMI
    (one device per process is the contract, include/cvlm.h; checked on the two heavy entries)."""
    if t.device.type != "cuda" or t.device.index != torch.cuda.current_device():
        raise RuntimeError(f"tensor on {t.device}, current device is cuda:{torch.cuda.current_device()}: call "
                           "torch.cuda.set_device() first (launches use the current device's stream)")


def gemm_workspace_bytes() -> int:
    return load().cvlm_gemm_workspace_bytes()


def new_gemm_workspace(device) -> torch.Tensor:
    """Zero-filled (the 4-KiB hand-off page must start at zero, include/cvlm.h) split-K workspace for cvlm_gemm."""
    return torch.zeros(gemm_workspace_bytes(), dtype=torch.uint8, device=device)


def gemm_workspace_errors(ws: torch.Tensor) -> int:
    """Abandoned split-K hand-offs (word 512) + rows a LayerNorm-folded launch refused (word 513) recorded in a workspace
    (synchronises).  Either kind has already turned the affected outputs into NaN.  0 in a healthy run."""
    words = ws[2048:2056].view(torch.int32).tolist()
    return int(words[0]) + int(words[1])


class H2IL:
    """Split-half activation in the 128-byte-row image of include/cvlm.h (ABI 6): one fp16 tensor [M][2 * C], row m =
    (hi c0..31 | lo c0..31 | hi c32..63 | lo c32..63 | ...).  Only cvlm_gemm (a_il / out_il / res_il) and cvlm_row_stats_split read or
    write it; `cols(c0)` is the view that starts at column c0 (c0 % 32 == 0) with the same row stride."""

    __slots__ = ("t",)
    il = True

    def __init__(self, t: torch.Tensor):
        assert t.dtype == torch.float16 and t.dim() == 2 and t.stride(1) == 1
        self.t = t

    @staticmethod
    def empty(M: int, C_: int, device="cuda") -> "H2IL":
        assert C_ % 32 == 0
        return H2IL(torch.empty(M, 2 * C_, dtype=torch.float16, device=device))

    @staticmethod
    def from_planes(x: "H2") -> "H2IL":
        return H2IL(interleave_planes(x))

    def cols(self, c0: int) -> "H2IL":
        assert c0 % 32 == 0
        return H2IL(self.t[:, 2 * c0:])

    def planes(self) -> "H2":
        M, C2 = self.t.shape
        return H2(self.t.reshape(M, C2 // 64, 2, 32).permute(2, 0, 1, 3).reshape(2, M, C2 // 2).contiguous())

    def float(self) -> torch.Tensor:
        return self.planes().float()


def mx_scale_pitch(C_: int) -> int:
    """Bytes per scale plane and row of an mx operand with C_ columns (include/cvlm.h ABI 10): one byte per 64-column group, padded to
    whole dwords (the kernel reads the bytes of four groups at once)."""
    return (C_ // 64 + 3) // 4 * 4


def mx_pack(x: "H2"):
    """h2 planes [2][R][C] (C % 64 == 0) -> (image uint8 [R][C / 64][256], scales uint8 [R][4][mx_scale_pitch(C)]) of include/cvlm.h
    ABI 10, in torch (weights at load time; the reference the tests hold the GEMM epilogue's own mx output against, bit for bit):
    per 32 columns E = max(exponent field of the largest |hi| as f32, 103) - 7, hi8 = e4m3(hi / 2^(E - 127)), lo8 = e4m3(lo / 2^(E - 138)).
    `lo` must be what the split leaves (|lo| <= half an ulp of its hi: H2.pack, every producer kernel): the lo8 scale is sized for that, and a
    plane of unrelated values overflows e4m3 (NaN bytes, as the hardware conversion gives)."""
    two, R, C_ = x.t.shape
    assert two == 2 and C_ % 64 == 0
    hi, lo = x.t[0], x.t[1]
    hf = hi.float()
    bmax = hf.abs().view(R, C_ // 32, 32).amax(-1)
    ex = ((bmax.view(torch.int32) >> 23) & 0xff).clamp_min(103) - 7                      # [R][C / 32]
    s_hi = (ex << 23).view(torch.float32)
    s_lo = ((ex - 11) << 23).view(torch.float32)
    hi8 = (hf.view(R, C_ // 32, 32) / s_hi[..., None]).to(torch.float8_e4m3fn).view(torch.uint8).view(R, C_ // 64, 64)
    lo8 = (lo.float().view(R, C_ // 32, 32) / s_lo[..., None]).to(torch.float8_e4m3fn).view(torch.uint8).view(R, C_ // 64, 64)
    img = torch.cat([hi.contiguous().view(torch.uint8).view(R, C_ // 64, 128), hi8, lo8], dim=2).contiguous()
    su = mx_scale_pitch(C_)
    sc = torch.zeros(R, 4, su, dtype=torch.uint8, device=x.t.device)
    e2 = ex.view(R, C_ // 64, 2).to(torch.uint8)
    sc[:, 0, :C_ // 64], sc[:, 1, :C_ // 64] = e2[:, :, 0], e2[:, :, 1]
    sc[:, 2, :C_ // 64], sc[:, 3, :C_ // 64] = e2[:, :, 0] - 11, e2[:, :, 1] - 11
    return img, sc


class H2MX:
    """Split-half activation as an mx operand (include/cvlm.h ABI 10): `t` uint8 [M][4 * C] -- per 64 columns 128 bytes of fp16 hi, 64
    of e4m3 hi8, 64 of e4m3 lo8 --, `s` uint8 [M][4][pitch] the block exponents, `lo` (optional) the fp16 lo PLANE [M][C] kept beside
    the image where a later launch reads the tensor as its h2 residual.  Written by cvlm_gemm (out_mx), read by it (a_mx / res_mx)."""

    __slots__ = ("t", "s", "lo", "C", "c0")
    mx = True

    def __init__(self, t: torch.Tensor, s: torch.Tensor, lo: Optional[torch.Tensor], C_: int, c0: int = 0):
        assert t.dtype == torch.uint8 and t.dim() == 2 and s.dtype == torch.uint8 and s.dim() == 3 and s.shape[1] == 4
        self.t, self.s, self.lo, self.C, self.c0 = t, s, lo, C_, c0

    @staticmethod
    def empty(M: int, C_: int, device="cuda", lo_plane: bool = False) -> "H2MX":
        assert C_ % 64 == 0
        return H2MX(torch.empty(M, 4 * C_, dtype=torch.uint8, device=device),
                    torch.zeros(M, 4, mx_scale_pitch(C_), dtype=torch.uint8, device=device),
                    torch.empty(M, C_, dtype=torch.float16, device=device) if lo_plane else None, C_)

    @staticmethod
    def from_planes(x: "H2", lo_plane: bool = False) -> "H2MX":
        img, sc = mx_pack(x)
        return H2MX(img.view(img.shape[0], -1), sc, x.t[1].contiguous() if lo_plane else None, x.t.shape[2])

    def cols(self, c0: int) -> "H2MX":
        """The operand that starts at column c0 (c0 % 64 == 0): same rows, same pitches."""
        assert c0 % 64 == 0 and self.lo is None
        return H2MX(self.t, self.s, None, self.C - c0, self.c0 + c0)

    def every(self, step: int) -> "H2MX":
        """Rows 0, step, 2 * step, ... as an operand of their own (views: same memory, `step` times the row pitches) -- the class-token
        rows of a [B * L]-row stream."""
        return H2MX(self.t[::step], self.s[::step], None if self.lo is None else self.lo[::step], self.C, self.c0)

    def data_ptr(self) -> int:
        return self.t.data_ptr() + 4 * self.c0

    def scale_ptr(self) -> int:
        return self.s.data_ptr() + self.c0 // 64

    def hi(self) -> torch.Tensor:
        M = self.t.shape[0]
        return self.t.view(M, -1, 256)[:, :, :128].contiguous().view(torch.float16).view(M, -1)[:, self.c0:self.c0 + self.C]

    def planes8(self):
        """(hi8, lo8) decoded to f32 [M][C]: what the fp8 products multiply."""
        M = self.t.shape[0]
        g = self.t.view(M, -1, 256)
        n = g.shape[1]
        e = self.s[:, :, :n].permute(0, 2, 1).float()                                     # [M][groups][4]
        dec = lambda b, pl: (b.contiguous().view(torch.float8_e4m3fn).float().view(M, n, 2, 32) *
                             torch.exp2(e[:, :, pl:pl + 2] - 127.0)[..., None]).view(M, -1)[:, self.c0:self.c0 + self.C]
        return dec(g[:, :, 128:192], 0), dec(g[:, :, 192:256], 2)


def interleave_planes(w: "H2") -> torch.Tensor:
    """[2][N][K] planes -> fp16 [N][2K] with row n = (hi k0..31 | lo k0..31 | hi k32..63 | lo k32..63 | ...): the `w_il` image of
    cvlm_gemm (include/cvlm.h, ABI 6).  K % 32 == 0."""
    two, N, K = w.t.shape
    assert two == 2 and K % 32 == 0
    return w.t.reshape(2, N, K // 32, 32).permute(1, 2, 0, 3).reshape(N, 2 * K).contiguous()


class H2:
    """Split-half tensor: two fp16 planes stored as one (2, *shape) fp16 tensor."""

    __slots__ = ("t",)

    def __init__(self, t: torch.Tensor):
        assert t.dtype == torch.float16 and t.shape[0] == 2
        self.t = t

    @staticmethod
    def empty(*shape, device="cuda") -> "H2":
        return H2(torch.empty((2,) + tuple(shape), dtype=torch.float16, device=device))

    @staticmethod
    def zeros(*shape, device="cuda") -> "H2":
        return H2(torch.zeros((2,) + tuple(shape), dtype=torch.float16, device=device))

    @staticmethod
    def pack(x: torch.Tensor) -> "H2":
        """Host-side (torch) packing of weights / constants: hi = fp16(x), lo = fp16(x - hi)."""
        x = x.float()
        hi = x.half()
        lo = (x - hi.float()).half()
        return H2(torch.stack([hi, lo]).contiguous())

    @property
    def hi(self) -> torch.Tensor:
        return self.t[0]

    @property
    def lo(self) -> torch.Tensor:
        return self.t[1]

    @property
    def shape(self):
        return self.t.shape[1:]

    def float(self) -> torch.Tensor:
        return self.t[0].float() + self.t[1].float()

    def view(self, *shape) -> "H2":
        return H2(self.t.view((2,) + tuple(shape)))


def gemm_args(a: H2, w: H2, M: int, N: int, K: int, *, lda: Optional[int] = None, ldw: Optional[int] = None,
              bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, ldr: Optional[int] = None,
              out_f32: Optional[torch.Tensor] = None, ldo: Optional[int] = None, out_h2: Optional[H2] = None,
              ldoh: Optional[int] = None, alpha: float = 1.0, act: int = ACT_NONE, split: int = 3, batch: int = 1,
              stride_a: int = 0, stride_w: int = 0, stride_r: int = 0, stride_o: int = 0, stride_oh: int = 0,
              pixel_shuffle: Optional[Tuple[int, int, int]] = None,
              head_major: Optional[Tuple[int, int, int]] = None, head_major_nolo: int = 0, out_scale: float = 1.0,
              workspace: Optional[torch.Tensor] = None,
              ln_fold: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
              residual_h2: Optional[Tuple["H2", float]] = None, ldrh: Optional[int] = None,
              row_stats: Optional[torch.Tensor] = None, conv3x3: Optional[Tuple[int, int, int]] = None,
              w_il: Optional[torch.Tensor] = None, w_mx: Optional["H2MX"] = None) -> GemmArgs:
    """w_mx: the weight as an mx operand (`H2MX.from_planes(w)`, ABI 10) -- used when `a` is an H2MX: hi.hi on fp16, the two correction
    products on the block-scaled e4m3 matrix instruction.  An H2MX `out_h2` / `residual_h2` selects out_mx / res_mx.
    w_il: the same weight with its planes interleaved per 32 k-elements (`interleave_planes(w)`, ABI 6): the big-tile kernels stage
    the weight from it (whole 128-byte lines per row and K-tile), same bits.
    conv3x3 = (H, W, C): `a` is an NHWC image [B*H*W][C] and K = 9*C runs over the taps of a 3x3 / pad 1 convolution
    (implicit GEMM: the im2col gather happens in the DMA addresses).
    ln_fold = (merged [M][2] f32 = (rstd, mu * rstd) from ln_stats_merge, colsum [N] f32): LayerNorm of the input folded into this
    GEMM (include/cvlm.h);
    residual_h2 = (x h2, scale): residual given as h2 planes; row_stats [ceil(N/64)][M][2] f32: piece statistics of the result rows
    (plain stores, bit-reproducible: nothing to zero)."""
    g = GemmArgs()
    if getattr(a, "mx", False):
        assert w_mx is not None and w_mx.C >= K and a.C >= K, "an mx activation needs the mx image of the weight"
        g.a_hi, g.a_lo, g.lda, g.stride_a, g.a_mx = a.data_ptr(), 0, a.t.stride(0) // 2, 0, 1
        assert a.s.stride(0) == 4 * a.s.stride(1), "an H2MX.every() view is a residual only: the kernels take the scale row stride as 4 * ld_s"
        g.a_mxs, g.lda_s = a.scale_ptr(), a.s.stride(1)
        g.w_mx, g.ldw_mx, g.w_mxs, g.ldw_s = w_mx.data_ptr(), w_mx.t.stride(0) // 2, w_mx.scale_ptr(), w_mx.s.stride(1)
    elif getattr(a, "il", False):
        g.a_hi, g.a_lo, g.lda, g.stride_a, g.a_il = a.t.data_ptr(), 0, a.t.stride(0), 0, 1
    else:
        g.a_hi, g.a_lo, g.lda, g.stride_a = a.hi.data_ptr(), a.lo.data_ptr(), lda if lda is not None else K, stride_a
    g.w_hi, g.w_lo, g.ldw, g.stride_w = w.hi.data_ptr(), w.lo.data_ptr(), ldw if ldw is not None else K, stride_w
    if w_il is not None:
        assert w_il.dtype == torch.float16 and w_il.dim() == 2 and w_il.shape[1] >= 2 * K and w_il.is_contiguous() and batch == 1
        g.w_il, g.ldw_il = w_il.data_ptr(), w_il.shape[1]
    g.bias = _p(bias)
    g.residual, g.ldr, g.stride_r = _p(residual), (ldr if ldr is not None else N), stride_r
    g.out_f32, g.ldo, g.stride_o = _p(out_f32), (ldo if ldo is not None else N), stride_o
    g.ldoh, g.stride_oh = (ldoh if ldoh is not None else N), stride_oh
    if out_h2 is not None and getattr(out_h2, "mx", False):
        g.out_hi, g.ldoh, g.out_mx = out_h2.data_ptr(), out_h2.t.stride(0) // 2, 1
        assert out_h2.s.stride(0) == 4 * out_h2.s.stride(1), "an H2MX.every() view is a residual only: the kernels take the scale row stride as 4 * ld_s"
        g.out_mxs, g.ldo_s = out_h2.scale_ptr(), out_h2.s.stride(1)
        if out_h2.lo is not None:
            g.out_lo, g.ldol = out_h2.lo.data_ptr(), out_h2.lo.stride(0)
    elif out_h2 is not None and getattr(out_h2, "il", False):
        g.out_hi, g.out_lo, g.ldoh, g.out_il = out_h2.t.data_ptr(), 0, out_h2.t.stride(0), 1
    elif out_h2 is not None:
        g.out_hi, g.out_lo = out_h2.hi.data_ptr(), out_h2.lo.data_ptr()
    g.M, g.N, g.K, g.batch = M, N, K, batch
    g.alpha, g.act, g.split = alpha, act, split
    if pixel_shuffle is not None:
        g.ps_h, g.ps_w, g.ps_c2 = pixel_shuffle
    if head_major is not None:
        g.hm_S, g.hm_H, g.hm_hd = head_major
        g.hm_nolo = head_major_nolo                                # ABI 12: bit w set = the lo plane of q (0) / k (1) / v (2) is not written
    g.out_scale = out_scale
    if ln_fold is not None:
        assert tuple(ln_fold[0].shape) == (M, 2) and ln_fold[0].is_contiguous(), "ln_fold: merged statistics [M][2]"
        g.ln_stats, g.ln_colsum = ln_fold[0].data_ptr(), ln_fold[1].data_ptr()
    if residual_h2 is not None:
        r, rs = residual_h2
        if getattr(r, "mx", False):
            assert r.lo is not None, "an mx residual needs its fp16 lo plane"
            g.res_hi, g.res_lo, g.ldrh, g.res_scale, g.res_mx = r.data_ptr(), r.lo.data_ptr(), r.t.stride(0) // 2, rs, 1
            g.ldrl = r.lo.stride(0)
        elif getattr(r, "il", False):
            g.res_hi, g.res_lo, g.ldrh, g.res_scale, g.res_il = r.t.data_ptr(), 0, r.t.stride(0), rs, 1
        else:
            g.res_hi, g.res_lo, g.ldrh, g.res_scale = r.hi.data_ptr(), r.lo.data_ptr(), (ldrh if ldrh is not None else N), rs
    if row_stats is not None:
        assert tuple(row_stats.shape) == (stats_pieces(N), M, 2) and row_stats.is_contiguous(), "row_stats: [pieces][M][2]"
        g.row_stats = row_stats.data_ptr()
    if conv3x3 is not None:
        g.conv_h, g.conv_w, g.conv_c = conv3x3
        g.lda = conv3x3[2]
    if workspace is not None:
        g.workspace, g.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    return g


@functools.wraps(gemm_args, assigned=("__doc__",))                 # help(), inspect.signature and editors show the parameter list above
def gemm(a: H2, w: H2, M: int, N: int, K: int, **kw) -> None:
    _on_current_device(a.t)
    _call("cvlm_gemm", gemm_args(a, w, M, N, K, **kw))


def gemm_plan(a: H2, w: H2, M: int, N: int, K: int, *, cus: int = 256, **kw) -> list:
    """Dry run of `gemm` with the same arguments on a device of `cus` compute units (cvlm_debug_gemm_plan: nothing is launched, no device
    is needed): one dict per launch -- kernel instantiation, grid, LDS bytes and the GemmParams fields csrc/gemm_plan.h chose."""
    g, info = gemm_args(a, w, M, N, K, **kw), GemmPlanInfo()
    have_ws = bool(g.workspace) and g.workspace_bytes >= gemm_workspace_bytes()
    _call("cvlm_debug_gemm_plan", g, int(have_ws), cus, info)
    return [dict({n: getattr(l, n) for n, _ in GemmLaunchInfo._fields_[:-1]}, kernel=l.kernel.decode())
            for l in info.launch[:info.launches]]


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, M: int, D: int, *,
              ldx: Optional[int] = None, add: Optional[torch.Tensor] = None, add_rows: int = 0,
              sum_out: Optional[torch.Tensor] = None, act: int = ACT_NONE, out_f32: Optional[torch.Tensor] = None,
              out_h2: Optional[H2] = None) -> None:
    _call("cvlm_layernorm", x.data_ptr(), ldx if ldx is not None else D, _p(add), add_rows, _p(sum_out), gamma.data_ptr(),
          beta.data_ptr(), eps, act, _p(out_f32), *_planes(out_h2), M, D)


def add_rows(a: torch.Tensor, b: Optional[torch.Tensor], b_rows: int, M: int, D: int, *, scale: float = 1.0,
             out_f32: Optional[torch.Tensor] = None, out_h2: Optional[H2] = None) -> None:
    _call("cvlm_add_rows", a.data_ptr(), _p(b), b_rows, scale, _p(out_f32), *_planes(out_h2), M, D)


def stats_pieces(D: int) -> int:
    """Piece planes of a row-statistics buffer for rows of D columns (include/cvlm.h: one (sum, centred squares) pair per 64 columns)."""
    return (D + 63) // 64


def ln_stats_merge(pieces: torch.Tensor, M: int, D: int, eps: float, merged: torch.Tensor,
                   workspace: Optional[torch.Tensor] = None) -> None:
    """pieces f32 [ceil(D/64)][rows >= M][2] (sum, centred sum of squares per 64 columns) -> merged f32 [M][2] = (rstd, mu * rstd):
    what `gemm(ln_fold=...)` reads.  workspace: a cvlm_gemm workspace whose error word counts refused rows."""
    assert pieces.dim() == 3 and pieces.shape[0] == stats_pieces(D) and pieces.shape[1] >= M and pieces.is_contiguous()
    assert tuple(merged.shape) == (M, 2) and merged.is_contiguous()
    _call("cvlm_ln_stats_merge", pieces.data_ptr(), pieces.shape[1], M, D, eps, merged.data_ptr(), _p(workspace))


def row_stats_split(x: torch.Tensor, scale: float, out: H2, stats: torch.Tensor, M: int, D: int, *, row0: int = 0,
                    copies: int = 1, dst_row_stride: int = 0) -> None:
    """out rows [row0 + c * dst_row_stride + m] = x[m] * scale as h2; stats f32 [pieces][rows][2] gets the piece statistics of the
    same rows (sum, centred sum of squares per 64 columns of the unscaled row)."""
    assert stats.dim() == 3 and stats.shape[0] == stats_pieces(D) and stats.shape[2] == 2 and stats.is_contiguous()
    if getattr(out, "mx", False):                                     # the rows as an mx operand (image + block exponents + lo plane), ABI 10
        assert out.lo is not None and out.c0 == 0 and out.C == D
        _call("cvlm_row_stats_split_mx", x.data_ptr(), scale, out.t.data_ptr() + row0 * out.t.stride(0), out.t.stride(0) // 2,
              out.s.data_ptr() + row0 * out.s.stride(0), out.s.stride(1), out.lo.data_ptr() + 2 * row0 * out.lo.stride(0),
              out.lo.stride(0), stats.data_ptr() + 8 * row0, stats.shape[1], M, D, copies, dst_row_stride)
        return
    _call("cvlm_row_stats_split", x.data_ptr(), scale, out.hi.data_ptr() + 2 * row0 * D, out.lo.data_ptr() + 2 * row0 * D,
          stats.data_ptr() + 8 * row0, stats.shape[1], M, D, copies, dst_row_stride)


def split_f32(x: torch.Tensor, out: H2) -> None:
    _call("cvlm_split_f32", x.data_ptr(), *_planes(out), x.numel())


def patchify(src0: torch.Tensor, src1: Optional[torch.Tensor], p: int, out: H2, ldk: int) -> None:
    B, C0, H, W = src0.shape
    C1 = 0 if src1 is None else src1.shape[1]
    _call("cvlm_patchify", src0.data_ptr(), C0, _p(src1), C1, B, H, W, p, *_planes(out), ldk)


def im2col3x3(x: torch.Tensor, B: int, H: int, W: int, Cc: int, out: H2) -> None:
    _call("cvlm_im2col3x3", x.data_ptr(), B, H, W, Cc, *_planes(out))


def reinterpret_transpose(x: torch.Tensor, B: int, T: int, D: int, out: H2, scale: float = 1.0) -> None:
    _call("cvlm_reinterpret_transpose", x.data_ptr(), B, T, D, scale, *_planes(out))


def attention(qkv: H2, out: H2, B: int, S: int, heads: int, hd: int, *, mode: int = 0, grid: int = 0, window: int = 0,
              causal: bool = False, pad: Optional[H2] = None, rel_h: Optional[H2] = None, rel_w: Optional[H2] = None,
              split_qk: int = 3, split_pv: int = 3, scale: Optional[float] = None, head_major: bool = False,
              workspace: Optional[torch.Tensor] = None, q_rows: int = 0) -> None:
    """q_rows > 0 (mode 0, ABI 9): only the first q_rows queries of every sequence (whole 128-query blocks are written).
    workspace: uint8 tensor of >= attention_workspace_bytes(...) bytes for the modes that need one; when omitted a
    temporary is taken from torch's allocator (stream-ordered, so it may be released right after the launch)."""
    _on_current_device(qkv.t)
    a = AttnArgs()
    a.qkv_hi, a.qkv_lo = qkv.hi.data_ptr(), qkv.lo.data_ptr()
    if pad is not None:
        a.pad_hi, a.pad_lo = pad.hi.data_ptr(), pad.lo.data_ptr()
    if rel_h is not None:
        a.relh_hi, a.relh_lo = rel_h.hi.data_ptr(), rel_h.lo.data_ptr()
        a.relw_hi, a.relw_lo = rel_w.hi.data_ptr(), rel_w.lo.data_ptr()
    a.out_hi, a.out_lo = out.hi.data_ptr(), out.lo.data_ptr()
    a.B, a.S, a.heads, a.hd = B, S, heads, hd
    a.mode, a.grid, a.window, a.causal = mode, grid, window, int(causal)
    a.split_qk, a.split_pv = split_qk, split_pv
    a.scale = float(hd) ** -0.5 if scale is None else scale
    a.qkv_layout = int(head_major)
    a.q_rows = q_rows
    need = load().cvlm_attention_workspace_bytes(a)
    if need > 0:
        if workspace is None or workspace.numel() * workspace.element_size() < need:
            workspace = torch.empty(need, dtype=torch.uint8, device=qkv.t.device)
        a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    _call("cvlm_attention", a)


def attention_reads_k_lo(mode: int, grid: int, window: int, hd: int, split_qk: int, split_pv: int, out_lo: bool = True) -> bool:
    """Whether cvlm_attention (csrc/attention.hip) reads K's lo plane for these arguments -- its dispatch restated.  False only where
    the kernel that runs takes no lo plane of K: split (1, 2) on the ViT-H kernels (64 x 64 / 96 x 96 global maps; 14 x 14 windows with
    an h2 output) and split (1, 1) everywhere.  (1, 2) on every other shape runs as (3, 3) and reads it; so does (3, 1).  A qkv
    projection may skip K's lo plane (cvlm_gemm_args.hm_nolo bit 1) only where this says False."""
    if (split_qk, split_pv) == (1, 1):
        return False
    if (split_qk, split_pv) != (1, 2):
        return True
    if mode == 1 and hd == 80:
        return grid not in (64, 96)
    if mode == 2 and hd == 80:
        return not (window == 14 and out_lo)
    return True


def attention_workspace_bytes(B: int, S: int, heads: int, hd: int, *, mode: int = 0, grid: int = 0, split_qk: int = 3,
                              split_pv: int = 3, **_unused) -> int:
    """Bytes of caller-owned scratch cvlm_attention wants for these arguments (0 for most modes)."""
    a = AttnArgs()
    a.B, a.S, a.heads, a.hd, a.mode, a.grid, a.split_qk, a.split_pv = B, S, heads, hd, mode, grid, split_qk, split_pv
    return load().cvlm_attention_workspace_bytes(a)


def small_attention(q, k, v, out, B: int, nq: int, nk: int, heads: int, hd: int, out_h2: Optional[H2] = None) -> None:
    """q f32 [B*nq][>= heads*hd], k / v f32 [B*nk][>= heads*hd]: 2-D tensors (or column blocks of one: the row pitch is taken from
    `.stride(0)`); out f32 [B*nq][heads*hd] and / or out_h2 planes of that shape."""
    ld = heads * hd
    pitch = lambda t: t.stride(-2) if t.dim() >= 2 else ld
    for t in (q, k, v):
        assert t.dtype == torch.float32 and t.stride(-1) == 1
    _call("cvlm_small_attention_h2", q.data_ptr(), pitch(q), k.data_ptr(), pitch(k), v.data_ptr(), pitch(v), _p(out), ld,
          *_planes(out_h2), ld, B, nq, nk, heads, hd)


def dense_pe(gauss: torch.Tensor, size: int, Cc: int, out: torch.Tensor) -> None:
    _call("cvlm_dense_pe", gauss.data_ptr(), size, Cc, out.data_ptr())


def mask_head(up, edge_emb, hyper, B: int, HW: int, Cc: int, low) -> None:
    _call("cvlm_mask_head", up.data_ptr(), _p(edge_emb), hyper.data_ptr(), B, HW, Cc, low.data_ptr())


def mask_head_edge(up, edge_emb, hyper, P: int, HW: int, Cc: int, low, edge_prob) -> None:
    """cvlm_mask_head for P prompts, also writing the edge probabilities edge_prob f32 [P][HW]."""
    _call("cvlm_mask_head_edge", up.data_ptr(), edge_emb.data_ptr(), hyper.data_ptr(), P, HW, Cc, low.data_ptr(), edge_prob.data_ptr())


def mask_head_multi(up, edge_emb, hyper, P: int, HW: int, Cc: int, n_masks: int, low, edge_prob=None) -> None:
    """low f32 [P][n_masks][HW] = masks 0..n_masks-1 of P prompts from one pass over up / edge_emb; edge_prob f32 [P][HW] (optional);
    edge_emb None: the plain hypernetwork products (include/cvlm.h)."""
    _call("cvlm_mask_head_multi", up.data_ptr(), _p(edge_emb), hyper.data_ptr(), P, HW, Cc, n_masks, low.data_ptr(), _p(edge_prob))


def topk_select(logits, B: int, Cc: int, K: int, txt, D: int, idx_in, idx_out, sel) -> None:
    """idx_out int64 [B][K] = the K largest logits per row, descending, ties to the lower index (or idx_in when given:
    gather only); sel f32 [B][K][D] = txt[idx_out] (include/cvlm.h)."""
    _call("cvlm_topk_select", _p(logits), B, Cc, K, txt.data_ptr(), D, _p(idx_in), idx_out.data_ptr(), sel.data_ptr())


def expand_blocks(image_of: torch.Tensor, P: int, B: int, block_elems: int, *, src_f32: Optional[torch.Tensor] = None,
                  dst_f32: Optional[torch.Tensor] = None, src_h2: Optional[H2] = None, dst_h2: Optional[H2] = None) -> None:
    """dst[p] = src[image_of[p]] for P blocks of block_elems contiguous elements out of B source blocks: an f32 pair, an h2 pair (both
    planes) or both in one launch, bit for bit (include/cvlm.h).  image_of int32 [P] on the device, entries in [0, B): the caller's
    contract."""
    assert image_of.dtype == torch.int32 and image_of.is_contiguous() and image_of.numel() >= P
    _call("cvlm_expand_blocks", image_of.data_ptr(), P, B, block_elems, _p(src_f32), _p(dst_f32), *_planes(src_h2), *_planes(dst_h2))


def bilinear(x, N: int, hin: int, win: int, out, hout: int, wout: int, sigmoid_in: bool = False) -> None:
    _call("cvlm_bilinear", x.data_ptr(), N, hin, win, out.data_ptr(), hout, wout, int(sigmoid_in))


def clip_assemble(patches, cls, pos, ctx, B: int, P: int, W: int, nctx: int, out) -> None:
    _call("cvlm_clip_assemble", patches.data_ptr(), cls.data_ptr(), pos.data_ptr(), ctx.data_ptr(), B, P, W, nctx, out.data_ptr())


def overwrite_rows(x, B: int, L: int, W: int, first: int, n: int, src) -> None:
    _call("cvlm_overwrite_rows", x.data_ptr(), B, L, W, first, n, src.data_ptr())


def gather_rows_h2(x: H2, scale: float, B: int, L: int, W: int, idx, fixed: int, out) -> None:
    """out[b] = (hi + lo)[b][idx[b] or fixed] * scale: one row per sequence of an h2 stream [B][L][W] as f32."""
    _call("cvlm_gather_rows_h2", *_planes(x), scale, B, L, W, _p(idx), fixed, out.data_ptr())


def gather_rows(x, B: int, L: int, W: int, idx, fixed: int, out) -> None:
    _call("cvlm_gather_rows", x.data_ptr(), B, L, W, _p(idx), fixed, out.data_ptr())


def clip_head(img, txt, logit_scale_exp: float, B: int, Cc: int, D: int, img_n, logits, pred, txt_sel) -> None:
    _call("cvlm_clip_head", img.data_ptr(), txt.data_ptr(), logit_scale_exp, B, Cc, D, img_n.data_ptr(), logits.data_ptr(),
          pred.data_ptr(), txt_sel.data_ptr())


def clip_head_wide_workspace_bytes(P: int, Cc: int) -> int:
    return _workspace_bytes("cvlm_clip_head_wide_workspace_bytes", P, Cc)


def clip_head_wide(img, txt, logit_scale_exp: float, P: int, Cc: int, D: int, img_n, logits, pred, txt_sel, workspace: torch.Tensor) -> None:
    """cvlm_clip_head for up to 65536 classes, tiled over classes (include/cvlm.h); workspace: uint8, at least
    clip_head_wide_workspace_bytes(P, Cc) bytes."""
    _call("cvlm_clip_head_wide", img.data_ptr(), txt.data_ptr(), logit_scale_exp, P, Cc, D, img_n.data_ptr(), logits.data_ptr(),
          pred.data_ptr(), txt_sel.data_ptr(), workspace.data_ptr(), workspace.numel() * workspace.element_size())


def topk_select_wide(logits, B: int, Cc: int, K: int, txt, D: int, idx_in, idx_out, sel) -> None:
    """topk_select's ranking for up to 65536 classes, K <= 64, under its signature; idx_in must be None (include/cvlm.h)."""
    _call("cvlm_topk_select_wide", logits.data_ptr(), B, Cc, K, txt.data_ptr(), D, _p(idx_in), idx_out.data_ptr(), sel.data_ptr())


def text_assemble(ids: Optional[torch.Tensor], table: Optional[torch.Tensor], emb: Optional[torch.Tensor], ctx: torch.Tensor,
                  pos: torch.Tensor, n: int, ctx_len: int, L: int, W: int, out: torch.Tensor) -> None:
    """out f32 [n][L][W] = [prefix | ctx | suffix] + pos of a vocabulary's prompts, from token ids (int32 [n][ctx_len]) and the
    embedding table or from embedded prompts f32 [n][ctx_len][W] (include/cvlm.h)."""
    assert ids is None or (ids.dtype == torch.int32 and ids.is_contiguous())
    _call("cvlm_text_assemble", _p(ids), _p(table), 0 if table is None else int(table.shape[0]), _p(emb), ctx.data_ptr(),
          int(ctx.shape[0]), pos.data_ptr(), n, ctx_len, L, W, out.data_ptr())


def normalize_add(x, add, R: int, D: int, out) -> None:
    _call("cvlm_normalize_add", x.data_ptr(), _p(add), R, D, out.data_ptr())


def resample_u8(src: torch.Tensor, bounds: torch.Tensor, kk: torch.Tensor, n_out: int, axis: int, dst: torch.Tensor) -> None:
    """src/dst uint8 [N][H][W][C]; bounds int32 [n_out][2]; kk int32 [n_out][ksize] (device tensors)."""
    N, H, W, Cc = src.shape
    _call("cvlm_resample_u8", src.data_ptr(), N, H, W, Cc, bounds.data_ptr(), kk.data_ptr(), kk.shape[1], n_out, axis, dst.data_ptr())


def u8_to_tensor(src: torch.Tensor, top: int, left: int, ch: int, cw: int, mean: torch.Tensor, std: torch.Tensor,
                 dst: torch.Tensor) -> None:
    N, H, W, Cc = src.shape
    _call("cvlm_u8_to_tensor", src.data_ptr(), N, H, W, Cc, top, left, ch, cw, mean.data_ptr(), std.data_ptr(), dst.data_ptr())


def mask_to_u8(logits: torch.Tensor, h: int, w: int, dst: torch.Tensor) -> None:
    """logits f32 [N][Hs][Ws] -> dst uint8 [N][h][w]: sigmoid, cv2-style bilinear resize, * 255, truncate."""
    N, Hs, Ws = logits.shape
    assert logits.dtype == torch.float32 and dst.dtype == torch.uint8 and tuple(dst.shape) == (N, h, w)
    assert logits.is_contiguous() and dst.is_contiguous()
    _call("cvlm_mask_to_u8", logits.data_ptr(), N, Hs, Ws, h, w, dst.data_ptr())


def mask_joint_hist(pre: torch.Tensor, gt: torch.Tensor, stats: torch.Tensor, hist: torch.Tensor) -> None:
    """pre/gt uint8 [N][h][w] -> stats int64 [N][3], hist int32 [N][4][2][256] (both overwritten)."""
    N, h, w = pre.shape
    assert pre.dtype == torch.uint8 and gt.dtype == torch.uint8 and tuple(gt.shape) == (N, h, w)
    assert stats.dtype == torch.int64 and tuple(stats.shape) == (N, 3) and hist.dtype == torch.int32
    assert tuple(hist.shape) == (N, 4, 2, 256) and pre.is_contiguous() and gt.is_contiguous()
    _call("cvlm_mask_joint_hist", pre.data_ptr(), gt.data_ptr(), N, h, w, stats.data_ptr(), hist.data_ptr())


# ---- packed masks and what is computed from them: every launcher below checks its tensors through `_check_tensors` and names its entry
# ---- through `_entry`; a device entry and its sequential host twin (include/cvlm.h: cvlm_debug_*_host) share one body `_x(host, ...)` under the two
# ---- public names, or one function with `host: bool` ----------------------------------------------------------------------------------------------------
_U8, _I16, _I32, _I64, _F32, _F64 = torch.uint8, torch.int16, torch.int32, torch.int64, torch.float32, torch.float64


def _check_tensors(like: torch.Tensor, *rows, optional=(), together=()) -> None:
    """The one argument check of the packed-mask launchers.  rows: (argument name, tensor, dtype, shape); every tensor must have that
    dtype and exactly that shape (a None element: any length; shape None: the caller checks it), be contiguous and live on `like`'s
    device.  None is allowed for the names in `optional` and for the members of the groups in `together`, each of which is given whole
    or not at all.  Raises AssertionError naming the argument, what was required and what came."""
    device, missing = like.device, []
    for name, t, dtype, shape in rows:
        if t is None:
            missing.append(name)
            continue
        got = t.shape
        assert (t.dtype == dtype and t.is_contiguous() and t.device == device and
                (got == shape or shape is None or (len(got) == len(shape) and all(w is None or w == g for w, g in zip(shape, got))))), \
            f"{name}: {dtype} {shape} contiguous on {device} required, got {t.dtype} {tuple(got)} strides {t.stride()} on {t.device}"
    for group in together:
        assert sum(name in missing for name in group) in (0, len(group)), f"{', '.join(group)}: given together or not at all"
    for name in missing:
        assert name in optional or any(name in group for group in together), f"{name}: required, got None"


def _entry(symbol: str, host: bool, like: torch.Tensor) -> str:
    """The entry a launcher calls, after the check of where its tensors live: the device entry `symbol` on the current device, or with
    host=True its twin cvlm_debug_<...>_host, which runs the kernels' per-thread functions sequentially on HOST tensors without a device."""
    if host:
        assert not like.is_cuda, f"{symbol}: the host form runs on host tensors, got one on {like.device}"
        return "cvlm_debug_" + symbol[5:] + "_host"
    _on_current_device(like)
    return symbol


def _sized_planes(bits, offsets, dims, prefix: str = "") -> int:
    """The check of a set of sized planes -- flat uint8 bits, byte offsets int64 [P + 1], dims int32 [P][2] = (h, w) -> P."""
    P = int(dims.shape[0])
    _check_tensors(bits, (prefix + "bits", bits, _U8, (None,)), (prefix + "offsets", offsets, _I64, (P + 1,)), (prefix + "dims", dims, _I32, (P, 2)))
    return P


def mask_pack(logits: torch.Tensor, bits: torch.Tensor, area: Optional[torch.Tensor] = None, box: Optional[torch.Tensor] = None) -> None:
    """logits f32 [P][H][W] -> bits uint8 [P][H * W / 8] in numpy.packbits' order (bit set iff logit > 0), area int32 [P], box int32
    [P][4] = inclusive (x0, y0, x1, y1), -1 for an empty plane; area and box together or not at all (include/cvlm.h)."""
    P, H, W = logits.shape
    assert (H * W) % 32 == 0
    _check_tensors(logits, ("logits", logits, _F32, (P, H, W)), ("bits", bits, _U8, (P, H * W // 8)), ("area", area, _I32, (P,)),
                   ("box", box, _I32, (P, 4)), together=(("area", "box"),))
    _on_current_device(logits)
    _call("cvlm_mask_pack", logits.data_ptr(), P, H * W, W, bits.data_ptr(), _p(area), _p(box))


def mask_overlap(bits: torch.Tensor, inter: torch.Tensor) -> None:
    """bits uint8 [n][K][bytes] (mask_pack's planes, bytes % 4 == 0) -> inter int32 [n][K][K] = popcount(plane a AND plane b) per
    image, the full symmetric matrix (overwritten; include/cvlm.h)."""
    n, K, nbytes = bits.shape
    assert nbytes % 4 == 0 and bits.data_ptr() % 4 == 0
    _check_tensors(bits, ("bits", bits, _U8, (n, K, nbytes)), ("inter", inter, _I32, (n, K, K)))
    _on_current_device(bits)
    _call("cvlm_mask_overlap", bits.data_ptr(), n, K, nbytes // 4, inter.data_ptr())


def mask_components_workspace_bytes(P: int, H: int, W: int) -> int:
    """Bytes cvlm_mask_components wants to keep all P planes of H x W in flight (14 per pixel and plane); P = 1: the minimum it takes."""
    return _workspace_bytes("cvlm_mask_components_workspace_bytes", P, H, W)


def _mask_components(host: bool, bits, H, W, connectivity, min_area, workspace, n_comp, comps=None, n_kept=None, kept_bits=None,
                     kept_area=None, kept_box=None) -> None:
    """The body of `mask_components` and of its host twin."""
    P, M = int(bits.shape[0]), 0 if comps is None else int(comps.shape[1])
    assert W % 32 == 0
    _check_tensors(bits, ("bits", bits, _U8, (P, H * W // 8)), ("workspace", workspace, _U8, (None,)), ("n_comp", n_comp, _I32, (P,)),
                   ("comps", comps, _I32, (P, M, 6)), ("n_kept", n_kept, _I32, (P,)), ("kept_bits", kept_bits, _U8, (P, H * W // 8)),
                   ("kept_area", kept_area, _I32, (P,)), ("kept_box", kept_box, _I32, (P, 4)),
                   optional=("comps", "workspace") if host else ("comps",), together=(("n_kept", "kept_bits", "kept_area", "kept_box"),))
    _call(_entry("cvlm_mask_components", host, bits), bits.data_ptr(), P, H, W, connectivity, M, min_area,
          *(() if host else (workspace.data_ptr(), workspace.numel())), n_comp.data_ptr(), _p(comps), _p(n_kept), _p(kept_bits), _p(kept_area),
          _p(kept_box))


def mask_components(bits: torch.Tensor, H: int, W: int, connectivity: int, min_area: int, workspace: torch.Tensor, n_comp: torch.Tensor,
                    comps: Optional[torch.Tensor] = None, n_kept: Optional[torch.Tensor] = None, kept_bits: Optional[torch.Tensor] = None,
                    kept_area: Optional[torch.Tensor] = None, kept_box: Optional[torch.Tensor] = None) -> None:
    """bits uint8 [P][H * W / 8] (mask_pack's planes) -> n_comp int32 [P], comps int32 [P][M][6] = (area, x0, y0, x1, y1, seed) of the M
    largest regions (M = comps.shape[1]; None: no table) and, with min_area >= 1, n_kept [P], kept_bits like bits, kept_area [P],
    kept_box [P][4] (all four or none).  workspace: uint8, at least mask_components_workspace_bytes(1, H, W) bytes; fewer than P planes'
    worth makes the entry walk the planes in rounds (include/cvlm.h)."""
    _mask_components(False, bits, H, W, connectivity, min_area, workspace, n_comp, comps, n_kept, kept_bits, kept_area, kept_box)


def mask_components_host(bits: torch.Tensor, H: int, W: int, connectivity: int, min_area: int, n_comp: torch.Tensor,
                         comps: Optional[torch.Tensor] = None, n_kept: Optional[torch.Tensor] = None, kept_bits: Optional[torch.Tensor] = None,
                         kept_area: Optional[torch.Tensor] = None, kept_box: Optional[torch.Tensor] = None) -> None:
    """`mask_components` on HOST tensors without a device (cvlm_debug_mask_components_host: the kernels' per-thread functions run
    sequentially on the CPU)."""
    _mask_components(True, bits, H, W, connectivity, min_area, None, n_comp, comps, n_kept, kept_bits, kept_area, kept_box)


def mask_holes_workspace_bytes(P: int, H: int, W: int) -> int:
    """Bytes cvlm_mask_holes wants to keep all P planes of H x W in flight (14 per pixel and plane); P = 1: the minimum it takes."""
    return _workspace_bytes("cvlm_mask_holes_workspace_bytes", P, H, W)


def _mask_holes(host: bool, bits, H, W, connectivity, fill_below, workspace, n_holes, holes=None, n_filled=None, filled_bits=None,
                filled_area=None) -> None:
    """The body of `mask_holes` and of its host twin."""
    P, M = int(bits.shape[0]), 0 if holes is None else int(holes.shape[1])
    assert W % 32 == 0
    _check_tensors(bits, ("bits", bits, _U8, (P, H * W // 8)), ("workspace", workspace, _U8, (None,)), ("n_holes", n_holes, _I32, (P,)),
                   ("holes", holes, _I32, (P, M, 6)), ("n_filled", n_filled, _I32, (P,)), ("filled_bits", filled_bits, _U8, (P, H * W // 8)),
                   ("filled_area", filled_area, _I32, (P,)),
                   optional=("holes", "workspace") if host else ("holes",), together=(("n_filled", "filled_bits", "filled_area"),))
    _call(_entry("cvlm_mask_holes", host, bits), bits.data_ptr(), P, H, W, connectivity, M, fill_below,
          *(() if host else (workspace.data_ptr(), workspace.numel())), n_holes.data_ptr(), _p(holes), _p(n_filled), _p(filled_bits),
          _p(filled_area))


def mask_holes(bits: torch.Tensor, H: int, W: int, connectivity: int, fill_below: int, workspace: torch.Tensor, n_holes: torch.Tensor,
               holes: Optional[torch.Tensor] = None, n_filled: Optional[torch.Tensor] = None, filled_bits: Optional[torch.Tensor] = None,
               filled_area: Optional[torch.Tensor] = None) -> None:
    """bits uint8 [P][H * W / 8] (mask_pack's planes) -> n_holes int32 [P], holes int32 [P][M][6] = (area, x0, y0, x1, y1, seed) of the M
    largest holes (M = holes.shape[1]; None: no table) and, with fill_below >= 1, n_filled [P], filled_bits like bits, filled_area [P]
    (all three or none).  connectivity is the FOREGROUND's; the clear pixels connect at its dual.  workspace: uint8, at least
    mask_holes_workspace_bytes(1, H, W) bytes; fewer than P planes' worth makes the entry walk the planes in rounds (include/cvlm.h)."""
    _mask_holes(False, bits, H, W, connectivity, fill_below, workspace, n_holes, holes, n_filled, filled_bits, filled_area)


def mask_holes_host(bits: torch.Tensor, H: int, W: int, connectivity: int, fill_below: int, n_holes: torch.Tensor,
                    holes: Optional[torch.Tensor] = None, n_filled: Optional[torch.Tensor] = None, filled_bits: Optional[torch.Tensor] = None,
                    filled_area: Optional[torch.Tensor] = None) -> None:
    """`mask_holes` on HOST tensors without a device (cvlm_debug_mask_holes_host: the kernels' per-thread functions run sequentially on
    the CPU)."""
    _mask_holes(True, bits, H, W, connectivity, fill_below, None, n_holes, holes, n_filled, filled_bits, filled_area)


def _mask_morph(host: bool, bits, H, W, radius, dil_bits=None, dil_area=None, ero_bits=None, ero_area=None, band_bits=None, band_area=None) -> None:
    """The body of `mask_morph` and of its host twin."""
    P, plane = int(bits.shape[0]), (int(bits.shape[0]), H * W // 8)
    assert W % 32 == 0
    _check_tensors(bits, ("bits", bits, _U8, plane), ("dil_bits", dil_bits, _U8, plane), ("dil_area", dil_area, _I32, (P,)),
                   ("ero_bits", ero_bits, _U8, plane), ("ero_area", ero_area, _I32, (P,)), ("band_bits", band_bits, _U8, plane),
                   ("band_area", band_area, _I32, (P,)), together=(("dil_bits", "dil_area"), ("ero_bits", "ero_area"), ("band_bits", "band_area")))
    _call(_entry("cvlm_mask_morph", host, bits), bits.data_ptr(), P, H, W, radius, _p(dil_bits), _p(dil_area), _p(ero_bits), _p(ero_area),
          _p(band_bits), _p(band_area))


def mask_morph(bits: torch.Tensor, H: int, W: int, radius: int, dil_bits: Optional[torch.Tensor] = None,
               dil_area: Optional[torch.Tensor] = None, ero_bits: Optional[torch.Tensor] = None, ero_area: Optional[torch.Tensor] = None,
               band_bits: Optional[torch.Tensor] = None, band_area: Optional[torch.Tensor] = None) -> None:
    """bits uint8 [P][H * W / 8] (mask_pack's planes) -> dilation, erosion and band = dil & ~ero by the (2 * radius + 1)^2 square, each
    a pair (planes like bits, popcount int32 [P]); a pair is given whole or not at all, at least one is asked for, and no output may
    overlap the input or another output.  Pixels outside the plane are clear to dilation and set to erosion (include/cvlm.h)."""
    _mask_morph(False, bits, H, W, radius, dil_bits, dil_area, ero_bits, ero_area, band_bits, band_area)


@functools.wraps(mask_morph, assigned=())        # help() and inspect.signature show the parameter list above
def mask_morph_host(*args, **kw) -> None:
    """`mask_morph` on HOST tensors without a device (cvlm_debug_mask_morph_host: the kernel's per-thread functions run sequentially on
    the CPU)."""
    _mask_morph(True, *args, **kw)


def _edge_pack(host: bool, prob, hout, wout, threshold, bits, area, with_bits=None, with_inter=None) -> None:
    """The body of `edge_pack` and of its host twin."""
    P, hin, win = (int(v) for v in prob.shape)
    assert wout % 32 == 0
    _check_tensors(prob, ("prob", prob, _F32, (P, hin, win)), ("bits", bits, _U8, (P, hout * wout // 8)), ("area", area, _I32, (P,)),
                   ("with_bits", with_bits, _U8, (P, hout * wout // 8)), ("with_inter", with_inter, _I32, (P,)),
                   together=(("with_bits", "with_inter"),))
    _call(_entry("cvlm_edge_pack", host, prob), prob.data_ptr(), P, hin, win, hout, wout, threshold, bits.data_ptr(), area.data_ptr(),
          _p(with_bits), _p(with_inter))


def edge_pack(prob: torch.Tensor, hout: int, wout: int, threshold: float, bits: torch.Tensor, area: torch.Tensor,
              with_bits: Optional[torch.Tensor] = None, with_inter: Optional[torch.Tensor] = None) -> None:
    """prob f32 [P][hin][win] -> bits uint8 [P][hout * wout / 8] in numpy.packbits' order, bit set iff the align_corners=False bilinear
    value at that output pixel -- float32, one rounding per operation -- is > threshold (0 < threshold < 1; NaN clear, +inf set), area
    int32 [P] = set bits; with_bits (planes like bits) and with_inter int32 [P] = popcount(bits & with_bits) together or not at all.
    No output may overlap an input or another output (include/cvlm.h)."""
    _edge_pack(False, prob, hout, wout, threshold, bits, area, with_bits, with_inter)


@functools.wraps(edge_pack, assigned=())        # help() and inspect.signature show the parameter list above
def edge_pack_host(*args, **kw) -> None:
    """`edge_pack` on HOST tensors without a device (cvlm_debug_edge_pack_host: the kernel's per-pixel functions run sequentially on
    the CPU)."""
    _edge_pack(True, *args, **kw)


def edge_pack_staged(hin: int, win: int, hout: int, wout: int) -> bool:
    """Whether cvlm_edge_pack runs these sizes through the instance that stages each tile's source footprint in LDS (True) or through
    the one that reads the planes directly (False): the launcher's own choice function (cvlm_debug_edge_pack_staged)."""
    rc = load().cvlm_debug_edge_pack_staged(hin, win, hout, wout)
    if rc < 0:
        raise RuntimeError(f"cvlm_debug_edge_pack_staged({hin}, {win}, {hout}, {wout}): sizes outside the entry's bounds")
    return bool(rc)


def mask_rle_workspace_bytes(P: int, H: int, W: int) -> int:
    """Bytes cvlm_mask_rle_emit wants to keep all P planes of H x W in flight (12 per 32 pixels and plane); P = 1: the minimum it takes."""
    return _workspace_bytes("cvlm_mask_rle_workspace_bytes", P, H, W)


def _rle(kind: str, bits, H: int, W: int, Wt: Optional[int], n_runs, offsets, counts, status, workspace) -> None:
    """The body of the run-length launchers: `kind` "count" (n_runs), "emit" (offsets, counts, status, workspace) or "host" (the merged
    host entry: n_runs and, all three or none, offsets, counts, status); Wt None: the planes' rows are full, otherwise the `_w` entry."""
    P = int(bits.shape[0])
    assert W % 32 == 0
    assert Wt is None or W - 32 < Wt <= W, "the true width ends inside the last word of the row pitch"
    _check_tensors(bits, ("bits", bits, _U8, (P, H * W // 8)), ("n_runs", n_runs, _I32, (P,)), ("offsets", offsets, _I64, (P + 1,)),
                   ("counts", counts, _I32, (None,)), ("status", status, _I32, (1,)), ("workspace", workspace, _U8, (None,)),
                   optional={"count": ("offsets", "counts", "status", "workspace"), "emit": ("n_runs",), "host": ("workspace",)}[kind],
                   together=(("offsets", "counts", "status"),) if kind == "host" else ())
    assert counts is None or counts.numel() >= 1
    w, wt = ("", ()) if Wt is None else ("_w", (Wt,))
    if kind == "host":
        assert not bits.is_cuda
        _call("cvlm_debug_mask_rle_host" + w, bits.data_ptr(), P, H, W, *wt, n_runs.data_ptr(), _p(offsets), _p(counts),
              0 if counts is None else counts.numel(), _p(status))
        return
    _on_current_device(bits)
    if kind == "count":
        _call("cvlm_mask_rle_count" + w, bits.data_ptr(), P, H, W, *wt, n_runs.data_ptr())
    else:
        _call("cvlm_mask_rle_emit" + w, bits.data_ptr(), P, H, W, *wt, offsets.data_ptr(), counts.data_ptr(), counts.numel(), status.data_ptr(),
              workspace.data_ptr(), workspace.numel())


def mask_rle_count(bits: torch.Tensor, H: int, W: int, n_runs: torch.Tensor) -> None:
    """bits uint8 [P][H * W / 8] (mask_pack's planes) -> n_runs int32 [P]: the counts of each plane's COCO run-length encoding
    (column-major, starting with the run of 0s; include/cvlm.h).  Two launches, no workspace."""
    _rle("count", bits, H, W, None, n_runs, None, None, None, None)


def mask_rle_emit(bits: torch.Tensor, H: int, W: int, offsets: torch.Tensor, counts: torch.Tensor, status: torch.Tensor,
                  workspace: torch.Tensor) -> None:
    """bits uint8 [P][H * W / 8] -> counts int32 [total]: plane p's run counts from counts[offsets[p]] on, inside its slice
    [offsets[p], offsets[p + 1]) (offsets int64 [P + 1], on the device); a count that would leave its slice or counts is dropped and
    status int32 [1] becomes 1, otherwise 0.  workspace: uint8, at least mask_rle_workspace_bytes(1, H, W) bytes; fewer than P planes'
    worth makes the entry walk the planes in rounds (include/cvlm.h)."""
    _rle("emit", bits, H, W, None, None, offsets, counts, status, workspace)


def mask_rle_host(bits: torch.Tensor, H: int, W: int, n_runs: torch.Tensor, offsets: Optional[torch.Tensor] = None,
                  counts: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None) -> None:
    """`mask_rle_count` and, with counts, `mask_rle_emit` on HOST tensors without a device (cvlm_debug_mask_rle_host: the kernels'
    per-thread functions run sequentially on the CPU)."""
    _rle("host", bits, H, W, None, n_runs, offsets, counts, status, None)


def mask_rle_count_w(bits: torch.Tensor, H: int, W: int, Wt: int, n_runs: torch.Tensor) -> None:
    """`mask_rle_count` of planes uint8 [P][H * W / 8] whose rows hold Wt <= W pixels, W - 32 < Wt (cvlm_mask_pack_sized's planes): the
    counts of the encoding of the H x Wt image (include/cvlm.h: cvlm_mask_rle_count_w)."""
    _rle("count", bits, H, W, Wt, n_runs, None, None, None, None)


def mask_rle_emit_w(bits: torch.Tensor, H: int, W: int, Wt: int, offsets: torch.Tensor, counts: torch.Tensor, status: torch.Tensor,
                    workspace: torch.Tensor) -> None:
    """`mask_rle_emit` of planes uint8 [P][H * W / 8] whose rows hold Wt <= W pixels (cvlm_mask_rle_emit_w); the workspace is
    mask_rle_workspace_bytes of the pitch W."""
    _rle("emit", bits, H, W, Wt, None, offsets, counts, status, workspace)


def mask_rle_host_w(bits: torch.Tensor, H: int, W: int, Wt: int, n_runs: torch.Tensor, offsets: Optional[torch.Tensor] = None,
                    counts: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None) -> None:
    """`mask_rle_count_w` and, with counts, `mask_rle_emit_w` on HOST tensors without a device (cvlm_debug_mask_rle_host_w)."""
    _rle("host", bits, H, W, Wt, n_runs, offsets, counts, status, None)


def _mask_pack_sized(host: bool, logits, dims, offsets, level, bits, max_words, area, box, status) -> None:
    """The body of `mask_pack_sized` and of its host twin."""
    P, Hs, Ws = logits.shape
    assert isinstance(level, int)
    _check_tensors(logits, ("logits", logits, _F32, (P, Hs, Ws)), ("dims", dims, _I32, (P, 2)), ("offsets", offsets, _I64, (P + 1,)),
                   ("bits", bits, _U8, (None,)), ("area", area, _I32, (P,)), ("box", box, _I32, (P, 4)), ("status", status, _I32, (1,)),
                   together=(("area", "box"),))
    _call(_entry("cvlm_mask_pack_sized", host, logits), logits.data_ptr(), P, Hs, Ws, dims.data_ptr(), offsets.data_ptr(), level,
          bits.data_ptr(), bits.numel(), int(max_words), _p(area), _p(box), status.data_ptr())


def mask_pack_sized(logits: torch.Tensor, dims: torch.Tensor, offsets: torch.Tensor, level: int, bits: torch.Tensor, max_words: int,
                    area: Optional[torch.Tensor], box: Optional[torch.Tensor], status: torch.Tensor) -> None:
    """logits f32 [P][Hs][Ws] -> the planes of `cvlm_mask_to_u8(...) >= level` at each plane's own size dims[p] = (h, w), packed as h rows of
    ceil(w / 32) words in numpy.packbits' order from byte offsets[p] of the flat uint8 tensor `bits` on (offsets int64 [P + 1]); area
    int32 [P] and box int32 [P][4] together or not at all; status int32 [1] becomes 1 if a plane's slice did not fit its size or left
    `bits` -- that plane is skipped --, otherwise 0.  max_words: the largest h * ceil(w / 32) of the call (include/cvlm.h)."""
    _mask_pack_sized(False, logits, dims, offsets, level, bits, max_words, area, box, status)


@functools.wraps(mask_pack_sized, assigned=())        # help() and inspect.signature show the parameter list above
def mask_pack_sized_host(*args, **kw) -> None:
    """`mask_pack_sized` on HOST tensors without a device (cvlm_debug_mask_pack_sized_host: the kernel's per-pixel functions run
    sequentially on the CPU)."""
    _mask_pack_sized(True, *args, **kw)


def mask_rle_decode_workspace_bytes(P: int, max_pixels: int) -> int:
    """Bytes cvlm_mask_rle_decode wants to keep all P planes of at most max_pixels pixels in flight (16 + one bit per pixel and plane);
    P = 1: the minimum it takes."""
    return _workspace_bytes("cvlm_mask_rle_decode_workspace_bytes", P, max_pixels)


def _mask_rle_decode(host: bool, counts, run_offsets, dims, bit_offsets, max_pixels, bits, area, box, status, workspace=None) -> None:
    """The body of `mask_rle_decode` and of its host twin."""
    P = int(dims.shape[0])
    _check_tensors(counts, ("counts", counts, _I32, (None,)), ("run_offsets", run_offsets, _I64, (P + 1,)), ("dims", dims, _I32, (P, 2)),
                   ("bit_offsets", bit_offsets, _I64, (P + 1,)), ("bits", bits, _U8, (None,)), ("area", area, _I32, (P,)),
                   ("box", box, _I32, (P, 4)), ("status", status, _I32, (1,)), ("workspace", workspace, _U8, (None,)),
                   optional=("workspace",) if host else (), together=(("area", "box"),))
    assert counts.numel() >= 1
    _call(_entry("cvlm_mask_rle_decode", host, counts), counts.data_ptr(), counts.numel(), run_offsets.data_ptr(), dims.data_ptr(),
          bit_offsets.data_ptr(), P, int(max_pixels), bits.data_ptr(), bits.numel(), _p(area), _p(box), status.data_ptr(),
          *(() if host else (workspace.data_ptr(), workspace.numel())))


def mask_rle_decode(counts: torch.Tensor, run_offsets: torch.Tensor, dims: torch.Tensor, bit_offsets: torch.Tensor, max_pixels: int,
                    bits: torch.Tensor, area: Optional[torch.Tensor], box: Optional[torch.Tensor], status: torch.Tensor,
                    workspace: torch.Tensor) -> None:
    """COCO run counts -> sized planes (include/cvlm.h: cvlm_mask_rle_decode): plane p's counts are counts[run_offsets[p] :
    run_offsets[p + 1]] (int32 [total], int64 [P + 1]), its size dims[p] = (h, w), and it is written as h rows of ceil(w / 32) words in
    numpy.packbits' order from byte bit_offsets[p] of the flat uint8 tensor `bits` on; area int32 [P] and box int32 [P][4] together or not
    at all.  status int32 [1] becomes 1 if a plane was refused -- counts that are negative or do not sum to h * w, a slice or a table that
    does not fit; such a plane is zero where its table holds and untouched where it does not --, otherwise 0.  max_pixels: the largest
    h * w of the call.  workspace: uint8, at least mask_rle_decode_workspace_bytes(1, max_pixels) bytes; fewer than P planes' worth makes
    the entry walk the planes in rounds."""
    _mask_rle_decode(False, counts, run_offsets, dims, bit_offsets, max_pixels, bits, area, box, status, workspace)


def mask_rle_decode_host(counts: torch.Tensor, run_offsets: torch.Tensor, dims: torch.Tensor, bit_offsets: torch.Tensor, max_pixels: int,
                         bits: torch.Tensor, area: Optional[torch.Tensor], box: Optional[torch.Tensor], status: torch.Tensor) -> None:
    """`mask_rle_decode` on HOST tensors without a device (cvlm_debug_mask_rle_decode_host: the kernels' per-thread functions run
    sequentially on the CPU)."""
    _mask_rle_decode(True, counts, run_offsets, dims, bit_offsets, max_pixels, bits, area, box, status)


def mask_poly_decode_workspace_bytes(P: int, max_pixels: int) -> int:
    """Bytes cvlm_mask_poly_decode wants to keep all P planes of at most max_pixels pixels in flight (two streams of 16 bytes + one bit
    per pixel per plane); P = 1: the minimum it takes."""
    return _workspace_bytes("cvlm_mask_poly_decode_workspace_bytes", P, max_pixels)


def _mask_poly_decode(host: bool, xy, poly_offsets, plane_polys, dims, bit_offsets, max_pixels, bits, area, box, status, workspace=None) -> None:
    """The body of `mask_poly_decode` and of its host twin."""
    P, Q = int(dims.shape[0]), int(poly_offsets.shape[0]) - 1
    _check_tensors(xy, ("xy", xy, _F64, (None,)), ("poly_offsets", poly_offsets, _I64, (Q + 1,)), ("plane_polys", plane_polys, _I32, (P + 1,)),
                   ("dims", dims, _I32, (P, 2)), ("bit_offsets", bit_offsets, _I64, (P + 1,)), ("bits", bits, _U8, (None,)),
                   ("area", area, _I32, (P,)), ("box", box, _I32, (P, 4)), ("status", status, _I32, (1,)), ("workspace", workspace, _U8, (None,)),
                   optional=("workspace",) if host else (), together=(("area", "box"),))
    assert xy.numel() >= 1 and Q >= 1
    _call(_entry("cvlm_mask_poly_decode", host, xy), xy.data_ptr(), xy.numel(), poly_offsets.data_ptr(), plane_polys.data_ptr(), dims.data_ptr(),
          bit_offsets.data_ptr(), P, Q, int(max_pixels), bits.data_ptr(), bits.numel(), _p(area), _p(box), status.data_ptr(),
          *(() if host else (workspace.data_ptr(), workspace.numel())))


def mask_poly_decode(xy: torch.Tensor, poly_offsets: torch.Tensor, plane_polys: torch.Tensor, dims: torch.Tensor, bit_offsets: torch.Tensor,
                     max_pixels: int, bits: torch.Tensor, area: Optional[torch.Tensor], box: Optional[torch.Tensor], status: torch.Tensor,
                     workspace: torch.Tensor) -> None:
    """COCO polygons -> sized planes (include/cvlm.h: cvlm_mask_poly_decode): polygon q is xy[poly_offsets[q] : poly_offsets[q + 1]]
    (float64 [total] = x0, y0, x1, y1, ...; int64 [Q + 1] in doubles), plane p the union of the polygons plane_polys[p] ..
    plane_polys[p + 1] - 1 (int32 [P + 1]) at the size dims[p] = (h, w), written like `mask_rle_decode`'s planes; area int32 [P] and box
    int32 [P][4] together or not at all.  status int32 [1] becomes 1 if a plane was refused -- a coordinate that is no finite number or
    beyond 65536, a polygon of fewer than 3 vertices or more than 2^24 walk points, a list, a slice or a table that does not fit; such a
    plane is zero where its table holds and untouched where it does not --, otherwise 0.  max_pixels: the largest h * w of the call.
    workspace: uint8, at least mask_poly_decode_workspace_bytes(1, max_pixels) bytes; fewer than P planes' worth makes the entry walk
    the planes in rounds."""
    _mask_poly_decode(False, xy, poly_offsets, plane_polys, dims, bit_offsets, max_pixels, bits, area, box, status, workspace)


def mask_poly_decode_host(xy: torch.Tensor, poly_offsets: torch.Tensor, plane_polys: torch.Tensor, dims: torch.Tensor,
                          bit_offsets: torch.Tensor, max_pixels: int, bits: torch.Tensor, area: Optional[torch.Tensor],
                          box: Optional[torch.Tensor], status: torch.Tensor) -> None:
    """`mask_poly_decode` on HOST tensors without a device (cvlm_debug_mask_poly_decode_host: the kernels' per-thread functions run
    sequentially on the CPU)."""
    _mask_poly_decode(True, xy, poly_offsets, plane_polys, dims, bit_offsets, max_pixels, bits, area, box, status)


def _mask_inter_sized(host: bool, a_bits, a_offsets, a_dims, b_bits, b_offsets, b_dims, pairs, max_words, inter, status) -> None:
    """The body of `mask_inter_sized` and of its host twin."""
    Pa, Pb, N = _sized_planes(a_bits, a_offsets, a_dims, "a_"), _sized_planes(b_bits, b_offsets, b_dims, "b_"), int(pairs.shape[0])
    _check_tensors(a_bits, ("b_bits", b_bits, _U8, (None,)), ("pairs", pairs, _I32, (N, 2)), ("inter", inter, _I32, (N,)),
                   ("status", status, _I32, (1,)))
    _call(_entry("cvlm_mask_inter_sized", host, a_bits), a_bits.data_ptr(), a_bits.numel(), a_offsets.data_ptr(), a_dims.data_ptr(), Pa,
          b_bits.data_ptr(), b_bits.numel(), b_offsets.data_ptr(), b_dims.data_ptr(), Pb, pairs.data_ptr(), N, int(max_words),
          inter.data_ptr(), status.data_ptr())


def mask_inter_sized(a_bits: torch.Tensor, a_offsets: torch.Tensor, a_dims: torch.Tensor, b_bits: torch.Tensor, b_offsets: torch.Tensor,
                     b_dims: torch.Tensor, pairs: torch.Tensor, max_words: int, inter: torch.Tensor, status: torch.Tensor) -> None:
    """Two sets of sized planes (flat uint8 bits, byte offsets int64 [P + 1], dims int32 [P][2]; they may be the same tensors) and pairs
    int32 [N][2] = (plane of A, plane of B) -> inter int32 [N] = |A[a] AND B[b]| over the columns below w (include/cvlm.h:
    cvlm_mask_inter_sized); a pair with an index out of range, a table that does not fit or two different sizes gives -1 and status
    int32 [1] = 1, otherwise 0.  max_words: the largest h * ceil(w / 32) of the call."""
    _mask_inter_sized(False, a_bits, a_offsets, a_dims, b_bits, b_offsets, b_dims, pairs, max_words, inter, status)


@functools.wraps(mask_inter_sized, assigned=())        # help() and inspect.signature show the parameter list above
def mask_inter_sized_host(*args, **kw) -> None:
    """`mask_inter_sized` on HOST tensors without a device (cvlm_debug_mask_inter_sized_host)."""
    _mask_inter_sized(True, *args, **kw)


def _coco_match(host: bool, boundary, det_offsets, gt_offsets, pair_offsets, inter, det_area, score, gt_area, gt_range_area, gt_crowd,
                iou_thrs, area_rngs, max_det, dt_order, dt_match, dt_ignore, gt_match, gt_ignore, status) -> None:
    """The body of `coco_match` (boundary None), of `coco_match_boundary` (boundary = (inter_b, det_area_b, gt_area_b)) and of their host twins."""
    E, N, ND, NG = int(det_offsets.numel()) - 1, int(inter.numel()), int(det_area.numel()), int(gt_area.numel())
    T, A = int(iou_thrs.numel()), int(area_rngs.shape[0])
    inter_b, det_area_b, gt_area_b = boundary or (None, None, None)
    _check_tensors(det_offsets, ("det_offsets", det_offsets, _I32, (E + 1,)), ("gt_offsets", gt_offsets, _I32, (E + 1,)),
                   ("pair_offsets", pair_offsets, _I64, (E + 1,)), ("inter", inter, _I32, (N,)), ("det_area", det_area, _I32, (ND,)),
                   ("score", score, _F32, (ND,)), ("gt_area", gt_area, _I32, (NG,)), ("gt_range_area", gt_range_area, _F64, (NG,)),
                   ("gt_crowd", gt_crowd, _U8, (NG,)), ("iou_thrs", iou_thrs, _F64, (T,)), ("area_rngs", area_rngs, _F64, (A, 2)),
                   ("inter_b", inter_b, _I32, (N,)), ("det_area_b", det_area_b, _I32, (ND,)), ("gt_area_b", gt_area_b, _I32, (NG,)),
                   ("dt_order", dt_order, _I32, (ND,)), ("dt_match", dt_match, _I32, (A, T, ND)), ("dt_ignore", dt_ignore, _U8, (A, T, ND)),
                   ("gt_match", gt_match, _I32, (A, T, NG)), ("gt_ignore", gt_ignore, _U8, (A, NG)), ("status", status, _I32, (1,)),
                   optional=() if boundary else ("inter_b", "det_area_b", "gt_area_b"))
    _call(_entry("cvlm_coco_match_boundary" if boundary else "cvlm_coco_match", host, det_offsets), det_offsets.data_ptr(), gt_offsets.data_ptr(),
          pair_offsets.data_ptr(), E, _pn(inter), N, _pn(det_area), _pn(score), ND, _pn(gt_area), _pn(gt_range_area), _pn(gt_crowd), NG,
          iou_thrs.data_ptr(), T, area_rngs.data_ptr(), A, int(max_det), *(_pn(t) for t in boundary or ()), _pn(dt_order), _pn(dt_match),
          _pn(dt_ignore), _pn(gt_match), _pn(gt_ignore), status.data_ptr())


def coco_match(det_offsets: torch.Tensor, gt_offsets: torch.Tensor, pair_offsets: torch.Tensor, inter: torch.Tensor, det_area: torch.Tensor,
               score: torch.Tensor, gt_area: torch.Tensor, gt_range_area: torch.Tensor, gt_crowd: torch.Tensor, iou_thrs: torch.Tensor,
               area_rngs: torch.Tensor, max_det: int, dt_order: torch.Tensor, dt_match: torch.Tensor, dt_ignore: torch.Tensor,
               gt_match: torch.Tensor, gt_ignore: torch.Tensor, status: torch.Tensor) -> None:
    """The COCO matching of E groups of detections and annotations (include/cvlm.h: cvlm_coco_match): offsets int32 /
    int32 / int64 [E + 1], inter int32 [N] in D_e x G_e blocks, det_area int32 and score f32 [sum D], gt_area int32, gt_range_area f64 and
    gt_crowd uint8 [sum G], iou_thrs f64 [T], area_rngs f64 [A][2] -> dt_order int32 [sum D], dt_match int32 and dt_ignore uint8 [A][T][sum D]
    in rank order, gt_match int32 [A][T][sum G], gt_ignore uint8 [A][sum G], status int32 [1] = 1 if a group was refused."""
    _coco_match(False, None, det_offsets, gt_offsets, pair_offsets, inter, det_area, score, gt_area, gt_range_area, gt_crowd, iou_thrs,
                area_rngs, max_det, dt_order, dt_match, dt_ignore, gt_match, gt_ignore, status)


@functools.wraps(coco_match, assigned=())        # help() and inspect.signature show the parameter list above
def coco_match_host(*args, **kw) -> None:
    """`coco_match` on HOST tensors without a device (cvlm_debug_coco_match_host: the same per-thread functions, run sequentially)."""
    _coco_match(True, None, *args, **kw)


def _coco_match_boundary(host: bool, det_offsets, gt_offsets, pair_offsets, inter, det_area, score, gt_area, gt_range_area, gt_crowd,
                         iou_thrs, area_rngs, max_det, inter_b, det_area_b, gt_area_b, dt_order, dt_match, dt_ignore, gt_match, gt_ignore,
                         status) -> None:
    """The body of `coco_match_boundary` and of its host twin."""
    _coco_match(host, (inter_b, det_area_b, gt_area_b), det_offsets, gt_offsets, pair_offsets, inter, det_area, score, gt_area, gt_range_area,
                gt_crowd, iou_thrs, area_rngs, max_det, dt_order, dt_match, dt_ignore, gt_match, gt_ignore, status)


def coco_match_boundary(det_offsets: torch.Tensor, gt_offsets: torch.Tensor, pair_offsets: torch.Tensor, inter: torch.Tensor,
                        det_area: torch.Tensor, score: torch.Tensor, gt_area: torch.Tensor, gt_range_area: torch.Tensor, gt_crowd: torch.Tensor,
                        iou_thrs: torch.Tensor, area_rngs: torch.Tensor, max_det: int, inter_b: torch.Tensor, det_area_b: torch.Tensor,
                        gt_area_b: torch.Tensor, dt_order: torch.Tensor, dt_match: torch.Tensor, dt_ignore: torch.Tensor,
                        gt_match: torch.Tensor, gt_ignore: torch.Tensor, status: torch.Tensor) -> None:
    """`coco_match` with the IoU of a pair replaced by min(mask IoU, boundary IoU) (include/cvlm.h: cvlm_coco_match_boundary; DESIGN.md
    §25): inter_b int32 [N], det_area_b int32 [sum D] and gt_area_b int32 [sum G] are the boundaries' intersections and areas, in the
    order of inter, det_area and gt_area."""
    _coco_match_boundary(False, det_offsets, gt_offsets, pair_offsets, inter, det_area, score, gt_area, gt_range_area, gt_crowd, iou_thrs,
                         area_rngs, max_det, inter_b, det_area_b, gt_area_b, dt_order, dt_match, dt_ignore, gt_match, gt_ignore, status)


@functools.wraps(coco_match_boundary, assigned=())        # help() and inspect.signature show the parameter list above
def coco_match_boundary_host(*args, **kw) -> None:
    """`coco_match_boundary` on HOST tensors without a device (cvlm_debug_coco_match_boundary_host)."""
    _coco_match_boundary(True, *args, **kw)


# ---- Boundary IoU ---------------------------------------------------------------------------------------------------------
def _mask_boundary_sized(host: bool, bits, offsets, dims, radius, max_words, workspace, out_bits, out_area, status) -> None:
    """The body of `mask_boundary_sized` and of its host twin."""
    P, n = _sized_planes(bits, offsets, dims), bits.numel()
    _check_tensors(bits, ("radius", radius, _I32, (P,)), ("workspace", workspace, _U8, (n,)), ("out_bits", out_bits, _U8, (n,)),
                   ("out_area", out_area, _I32, (P,)), ("status", status, _I32, (1,)), optional=("out_area",))
    _call(_entry("cvlm_mask_boundary_sized", host, bits), bits.data_ptr(), n, offsets.data_ptr(), dims.data_ptr(), radius.data_ptr(), P,
          int(max_words), workspace.data_ptr(), out_bits.data_ptr(), _p(out_area), status.data_ptr())


def mask_boundary_sized(bits: torch.Tensor, offsets: torch.Tensor, dims: torch.Tensor, radius: torch.Tensor, max_words: int,
                        workspace: torch.Tensor, out_bits: torch.Tensor, out_area: Optional[torch.Tensor], status: torch.Tensor) -> None:
    """The boundary of each sized plane at its own radius (include/cvlm.h: cvlm_mask_boundary_sized): bits flat uint8,
    byte offsets int64 [P + 1], dims int32 [P][2], radius int32 [P] in 1 .. 16384 -> out_bits (the same layout, X & ~erode(X, radius) with
    the outside of the plane clear), out_area int32 [P] or None, status int32 [1] = 1 if a plane was refused.  workspace: uint8, as
    many bytes as bits.  max_words: the largest h * ceil(w / 32) of the call."""
    _mask_boundary_sized(False, bits, offsets, dims, radius, max_words, workspace, out_bits, out_area, status)


@functools.wraps(mask_boundary_sized, assigned=())        # help() and inspect.signature show the parameter list above
def mask_boundary_sized_host(*args, **kw) -> None:
    """`mask_boundary_sized` on HOST tensors without a device (cvlm_debug_mask_boundary_sized_host: the kernels' per-thread functions
    run sequentially)."""
    _mask_boundary_sized(True, *args, **kw)


# ---- Contours: COCO polygons out ------------------------------------------------------------------------------------------
def _contour_outputs(P: int, like, vertex_offsets, xy, ring_start, n_rings, all_or_none: bool = False) -> int:
    """The check of the outputs of the contour emit (all_or_none: the host entry, which only counts without them) -> total."""
    total = 0 if xy is None else int(xy.shape[0])
    _check_tensors(like, ("vertex_offsets", vertex_offsets, _I64, (P + 1,)), ("xy", xy, _I16, (total, 2)), ("ring_start", ring_start, _U8, (total,)),
                   ("n_rings", n_rings, _I32, (P, 2)), together=(("vertex_offsets", "xy", "ring_start", "n_rings"),) if all_or_none else ())
    return total


def mask_contour_workspace_bytes(P: int, round_vertices: int, max_words: int) -> int:
    """Bytes of workspace of one `mask_contour_emit` call on P planes that hold round_vertices vertices together (host arithmetic)."""
    return _workspace_bytes("cvlm_mask_contour_workspace_bytes", P, round_vertices, max_words)


def mask_contour_count(bits: torch.Tensor, offsets: torch.Tensor, dims: torch.Tensor, connectivity: int, max_words: int,
                       n_vertices: torch.Tensor, status: torch.Tensor) -> None:
    """Vertices of the crack contour of each sized plane (include/cvlm.h: cvlm_mask_contour_count): bits flat uint8, byte
    offsets int64 [P + 1], dims int32 [P][2] -> n_vertices int32 [P], status int32 [1] = 1 if a plane was refused."""
    P = _sized_planes(bits, offsets, dims)
    _check_tensors(bits, ("n_vertices", n_vertices, _I32, (P,)), ("status", status, _I32, (1,)))
    _on_current_device(bits)
    _call("cvlm_mask_contour_count", bits.data_ptr(), bits.numel(), offsets.data_ptr(), dims.data_ptr(), P, int(connectivity), int(max_words),
          n_vertices.data_ptr(), status.data_ptr())


def mask_contour_emit(bits: torch.Tensor, offsets: torch.Tensor, dims: torch.Tensor, connectivity: int, max_words: int,
                      vertex_offsets: torch.Tensor, round_vertices: int, xy: torch.Tensor, ring_start: torch.Tensor, n_rings: torch.Tensor,
                      status: torch.Tensor, workspace: torch.Tensor) -> None:
    """The rings of each sized plane (include/cvlm.h: cvlm_mask_contour_emit).  offsets / dims / vertex_offsets / n_rings
    may be views of longer tables -- one round of planes of a larger call --; xy int16 [total][2] and ring_start uint8 [total] are whole
    and vertex_offsets absolute.  round_vertices: at least the vertices of these planes."""
    P = _sized_planes(bits, offsets, dims)
    total = _contour_outputs(P, bits, vertex_offsets, xy, ring_start, n_rings)
    _check_tensors(bits, ("status", status, _I32, (1,)), ("workspace", workspace, _U8, (None,)))
    _on_current_device(bits)
    _call("cvlm_mask_contour_emit", bits.data_ptr(), bits.numel(), offsets.data_ptr(), dims.data_ptr(), P, int(connectivity), int(max_words),
          vertex_offsets.data_ptr(), int(round_vertices), _pn(xy), _pn(ring_start), n_rings.data_ptr(), total, status.data_ptr(),
          workspace.data_ptr(), workspace.numel())


def mask_contour_host(bits: torch.Tensor, offsets: torch.Tensor, dims: torch.Tensor, connectivity: int, n_vertices: torch.Tensor,
                      status: torch.Tensor, vertex_offsets: Optional[torch.Tensor] = None, xy: Optional[torch.Tensor] = None,
                      ring_start: Optional[torch.Tensor] = None, n_rings: Optional[torch.Tensor] = None) -> None:
    """`mask_contour_count` (vertex_offsets, xy, ring_start and n_rings None) or count and emit (all four) on HOST tensors without a device
    (cvlm_debug_mask_contour_host: the kernels' maps and successors, the rings followed sequentially)."""
    P = _sized_planes(bits, offsets, dims)
    _check_tensors(bits, ("n_vertices", n_vertices, _I32, (P,)), ("status", status, _I32, (1,)))
    total = _contour_outputs(P, bits, vertex_offsets, xy, ring_start, n_rings, all_or_none=True)
    assert not bits.is_cuda
    _call("cvlm_debug_mask_contour_host", bits.data_ptr(), bits.numel(), offsets.data_ptr(), dims.data_ptr(), P, int(connectivity),
          n_vertices.data_ptr(), _p(vertex_offsets), _pn(xy), _pn(ring_start), _p(n_rings), total, status.data_ptr())


# ---- Simplified contour rings: Douglas-Peucker polygons out ----------------------------------------------------------------
def _simplify_rings(xy, ring_start, vertex_offsets) -> Tuple[int, int]:
    """The check of the rings a simplify entry reads -- xy int16 [total][2], ring_start uint8 [total], vertex_offsets int64 [P + 1], a
    view of a longer table allowed -> (P, total)."""
    P, total = int(vertex_offsets.shape[0]) - 1, int(xy.shape[0])
    assert P >= 1, f"vertex_offsets: one entry more than planes, got {tuple(vertex_offsets.shape)}"
    _check_tensors(xy, ("xy", xy, _I16, (total, 2)), ("ring_start", ring_start, _U8, (total,)), ("vertex_offsets", vertex_offsets, _I64, (P + 1,)))
    return P, total


def _simplify_marks(P: int, total: int, like, T, keep, n_kept, n_rings_out, status) -> None:
    _check_tensors(like, ("T", T, _I32, (P,)), ("keep", keep, _U8, (total,)), ("n_kept", n_kept, _I32, (P,)),
                   ("n_rings_out", n_rings_out, _I32, (P, 2)), ("status", status, _I32, (1,)))


def _simplify_outputs(P: int, like, out_offsets, xy_out, ring_start_out, all_or_none: bool = False) -> int:
    """The check of the outputs of the simplify emit (all_or_none: the host entry, which only marks without them) -> total_out."""
    total_out = 0 if xy_out is None else int(xy_out.shape[0])
    _check_tensors(like, ("out_offsets", out_offsets, _I64, (P + 1,)), ("xy_out", xy_out, _I16, (total_out, 2)),
                   ("ring_start_out", ring_start_out, _U8, (total_out,)),
                   together=(("out_offsets", "xy_out", "ring_start_out"),) if all_or_none else ())
    return total_out


def contour_simplify_workspace_bytes(P: int, round_vertices: int) -> int:
    """Bytes of workspace of one `contour_simplify_mark` call on P planes that hold round_vertices vertices together (host arithmetic)."""
    return _workspace_bytes("cvlm_contour_simplify_workspace_bytes", P, round_vertices)


def contour_simplify_mark(xy: torch.Tensor, ring_start: torch.Tensor, vertex_offsets: torch.Tensor, T: torch.Tensor, round_vertices: int,
                          keep: torch.Tensor, n_kept: torch.Tensor, n_rings_out: torch.Tensor, status: torch.Tensor,
                          workspace: torch.Tensor) -> None:
    """Which vertices of each plane's rings Ramer-Douglas-Peucker keeps (include/cvlm.h: cvlm_contour_simplify_mark): xy
    int16 [total][2], ring_start uint8 [total], vertex_offsets int64 [P + 1], T int32 [P] in quarter pixels -> keep uint8 [total], n_kept
    int32 [P], n_rings_out int32 [P][2], status int32 [1] = 1 if a plane was refused.  vertex_offsets / T / n_kept / n_rings_out may be
    views of longer tables -- one round of planes of a larger call --; xy, ring_start and keep are whole and vertex_offsets absolute.
    round_vertices: at least the vertices of these planes."""
    P, total = _simplify_rings(xy, ring_start, vertex_offsets)
    _simplify_marks(P, total, xy, T, keep, n_kept, n_rings_out, status)
    _check_tensors(xy, ("workspace", workspace, _U8, (None,)))
    _call(_entry("cvlm_contour_simplify_mark", False, xy), _pn(xy), _pn(ring_start), vertex_offsets.data_ptr(), total, T.data_ptr(), P,
          int(round_vertices), _pn(keep), n_kept.data_ptr(), n_rings_out.data_ptr(), status.data_ptr(), workspace.data_ptr(), workspace.numel())


def contour_simplify_emit(xy: torch.Tensor, ring_start: torch.Tensor, vertex_offsets: torch.Tensor, keep: torch.Tensor,
                          out_offsets: torch.Tensor, xy_out: torch.Tensor, ring_start_out: torch.Tensor, status: torch.Tensor) -> None:
    """The kept vertices of each plane, in order (include/cvlm.h: cvlm_contour_simplify_emit): plane p's go to the entries
    [out_offsets[p], out_offsets[p + 1]) of xy_out int16 [total_out][2] and ring_start_out uint8 [total_out] (1 outer ring, 2 hole)."""
    P, total = _simplify_rings(xy, ring_start, vertex_offsets)
    total_out = _simplify_outputs(P, xy, out_offsets, xy_out, ring_start_out)
    _check_tensors(xy, ("keep", keep, _U8, (total,)), ("status", status, _I32, (1,)))
    _call(_entry("cvlm_contour_simplify_emit", False, xy), _pn(xy), _pn(ring_start), vertex_offsets.data_ptr(), total, _pn(keep), P,
          out_offsets.data_ptr(), _pn(xy_out), _pn(ring_start_out), total_out, status.data_ptr())


def contour_simplify_sequential(xy: torch.Tensor, ring_start: torch.Tensor, vertex_offsets: torch.Tensor, T: torch.Tensor, keep: torch.Tensor,
                                n_kept: torch.Tensor, n_rings_out: torch.Tensor, status: torch.Tensor,
                                out_offsets: Optional[torch.Tensor] = None, xy_out: Optional[torch.Tensor] = None,
                                ring_start_out: Optional[torch.Tensor] = None) -> None:
    """`contour_simplify_mark` (out_offsets, xy_out and ring_start_out None) or mark and emit (all three) on HOST tensors without a device
    (cvlm_debug_contour_simplify_host: a sequential recursion with an explicit stack over the kernels' key, keep test and anchor rule)."""
    P, total = _simplify_rings(xy, ring_start, vertex_offsets)
    _simplify_marks(P, total, xy, T, keep, n_kept, n_rings_out, status)
    total_out = _simplify_outputs(P, xy, out_offsets, xy_out, ring_start_out, all_or_none=True)
    _call(_entry("cvlm_contour_simplify", True, xy), _pn(xy), _pn(ring_start), vertex_offsets.data_ptr(), total, T.data_ptr(), P, _pn(keep),
          n_kept.data_ptr(), n_rings_out.data_ptr(), _p(out_offsets), _pn(xy_out), _pn(ring_start_out), total_out, status.data_ptr())


# ---- Distance maps and surface totals --------------------------------------------------------------------------------------
DT_FAR = 0x7fffffff               # D2 of a pixel with no set pixel within reach (csrc/distance_logic.h)


def mask_distance_workspace_bytes(P: int, max_pixels: int) -> int:
    """Bytes of workspace that hold `mask_distance_sized` on P planes of at most max_pixels pixels lying back to back (host arithmetic)."""
    return _workspace_bytes("cvlm_mask_distance_workspace_bytes", P, max_pixels)


def mask_surface_workspace_bytes(N: int) -> int:
    """Bytes of workspace of one `mask_surface_totals` call on N pairs (host arithmetic)."""
    return _workspace_bytes("cvlm_mask_surface_workspace_bytes", N)


def _mask_distance_sized(host: bool, bits, offsets, dims, reach, max_words, pix_offsets, workspace, out_d2, status) -> None:
    """The body of `mask_distance_sized` and of its host twin."""
    P = _sized_planes(bits, offsets, dims)
    _check_tensors(bits, ("reach", reach, _I32, (P,)), ("pix_offsets", pix_offsets, _I64, (P + 1,)), ("workspace", workspace, _U8, (None,)),
                   ("out_d2", out_d2, _I32, (None,)), ("status", status, _I32, (1,)))
    assert out_d2.numel() >= 1
    _call(_entry("cvlm_mask_distance_sized", host, bits), bits.data_ptr(), bits.numel(), offsets.data_ptr(), dims.data_ptr(), reach.data_ptr(), P,
          int(max_words), pix_offsets.data_ptr(), out_d2.numel(), workspace.data_ptr(), workspace.numel(), out_d2.data_ptr(), status.data_ptr())


def mask_distance_sized(bits: torch.Tensor, offsets: torch.Tensor, dims: torch.Tensor, reach: torch.Tensor, max_words: int,
                        pix_offsets: torch.Tensor, workspace: torch.Tensor, out_d2: torch.Tensor, status: torch.Tensor) -> None:
    """The squared distance map of each sized plane (include/cvlm.h: cvlm_mask_distance_sized): bits flat uint8, byte
    offsets int64 [P + 1], dims int32 [P][2], reach int32 [P] in 0 .. 23170 (0: unlimited) -> out_d2 int32 [n_pix], plane p's h * w
    values at pix_offsets[p] (int64 [P + 1], in pixels), DT_FAR where no set pixel is within reach; status int32 [1] = 1 if a plane was
    refused.  workspace: uint8, 2 bytes per entry of out_d2 rounded up to 16.  max_words: the largest h * ceil(w / 32) of the call."""
    _mask_distance_sized(False, bits, offsets, dims, reach, max_words, pix_offsets, workspace, out_d2, status)


@functools.wraps(mask_distance_sized, assigned=())        # help() and inspect.signature show the parameter list above
def mask_distance_sized_host(*args, **kw) -> None:
    """`mask_distance_sized` on HOST tensors without a device (cvlm_debug_mask_distance_sized_host: the kernels' per-thread functions
    run sequentially)."""
    _mask_distance_sized(True, *args, **kw)


def _mask_surface_totals(host: bool, a_bits, a_offsets, a_dims, b_d2, b_pix_offsets, b_dims, pairs, radii, max_words, workspace, n, far,
                         within, max_d2, sum_d2, sum_d, status) -> None:
    """The body of `mask_surface_totals` and of its host twin."""
    Pa, Pb = _sized_planes(a_bits, a_offsets, a_dims, "a_"), int(b_dims.shape[0])
    N, T = int(pairs.shape[0]), int(radii.shape[-1])
    _check_tensors(a_bits, ("b_d2", b_d2, _I32, (None,)), ("b_pix_offsets", b_pix_offsets, _I64, (Pb + 1,)), ("b_dims", b_dims, _I32, (Pb, 2)),
                   ("pairs", pairs, _I32, (N, 2)), ("radii", radii, _I32, (N, T)), ("workspace", workspace, _U8, (None,)), ("n", n, _I32, (N,)),
                   ("far", far, _I32, (N,)), ("within", within, _I32, (N, T)), ("max_d2", max_d2, _I32, (N,)), ("sum_d2", sum_d2, _I64, (N,)),
                   ("sum_d", sum_d, _F64, (N,)), ("status", status, _I32, (1,)))
    _call(_entry("cvlm_mask_surface_totals", host, a_bits), a_bits.data_ptr(), a_bits.numel(), a_offsets.data_ptr(), a_dims.data_ptr(), Pa,
          b_d2.data_ptr(), b_pix_offsets.data_ptr(), b_d2.numel(), b_dims.data_ptr(), Pb, pairs.data_ptr(), N, radii.data_ptr(), T,
          int(max_words), workspace.data_ptr(), workspace.numel(), n.data_ptr(), far.data_ptr(), within.data_ptr(), max_d2.data_ptr(),
          sum_d2.data_ptr(), sum_d.data_ptr(), status.data_ptr())


def mask_surface_totals(a_bits: torch.Tensor, a_offsets: torch.Tensor, a_dims: torch.Tensor, b_d2: torch.Tensor, b_pix_offsets: torch.Tensor,
                        b_dims: torch.Tensor, pairs: torch.Tensor, radii: torch.Tensor, max_words: int, workspace: torch.Tensor,
                        n: torch.Tensor, far: torch.Tensor, within: torch.Tensor, max_d2: torch.Tensor, sum_d2: torch.Tensor,
                        sum_d: torch.Tensor, status: torch.Tensor) -> None:
    """Directed surface totals of pairs (include/cvlm.h: cvlm_mask_surface_totals): over the set pixels of plane
    pairs[i, 0] of A (sized planes) against map pairs[i, 1] of B (`mask_distance_sized`'s out_d2, pix_offsets and dims) -> n, far, max_d2
    int32 [N], within int32 [N][T] at radii int32 [N][T], sum_d2 int64 [N], sum_d float64 [N]; status int32 [1] = 1 if a pair was refused
    (-1 in its integers).  workspace: uint8, `mask_surface_workspace_bytes(N)`."""
    _mask_surface_totals(False, a_bits, a_offsets, a_dims, b_d2, b_pix_offsets, b_dims, pairs, radii, max_words, workspace, n, far, within,
                         max_d2, sum_d2, sum_d, status)


@functools.wraps(mask_surface_totals, assigned=())        # help() and inspect.signature show the parameter list above
def mask_surface_totals_host(*args, **kw) -> None:
    """`mask_surface_totals` on HOST tensors without a device (cvlm_debug_mask_surface_totals_host)."""
    _mask_surface_totals(True, *args, **kw)


# ---- Thinning: skeletons, thin edges, clDice ----------------------------------------------------------------------------------
THIN_MAX_ITER = 1 << 30           # max_iter of a plane: 0 (no limit) .. 2^30 (csrc/thin_logic.h: TH_MAX_ITER)
THIN_MAX_STEPS = 1024             # iterations the stepping path launches in one call (TH_MAX_STEPS)


def mask_thin_workspace_bytes(n_bytes: int, P: int, steps: int) -> int:
    """Bytes of workspace of one `mask_thin_sized` call on P planes of n_bytes bytes in all with `steps` stepped iterations (host
    arithmetic): the stepped state plus the flags."""
    return _workspace_bytes("cvlm_mask_thin_workspace_bytes", n_bytes, P, steps)


def mask_thin_resident(h: int, w: int) -> bool:
    """Whether an h x w plane, with its clear border, fits the resident kernel's LDS budget (host arithmetic: cvlm_mask_thin_resident)."""
    return bool(load().cvlm_mask_thin_resident(int(h), int(w)))


def _mask_thin_sized(host: bool, bits, offsets, dims, max_iter, max_words, mode, steps, workspace, out_bits, out_area, out_box, out_iters,
                     out_done, status) -> None:
    """The body of `mask_thin_sized` and of its host twin."""
    P = _sized_planes(bits, offsets, dims)
    _check_tensors(bits, ("max_iter", max_iter, _I32, (P,)), ("workspace", workspace, _U8, (None,)), ("out_bits", out_bits, _U8, (bits.numel(),)),
                   ("out_area", out_area, _I32, (P,)), ("out_box", out_box, _I32, (P, 4)), ("out_iters", out_iters, _I32, (P,)),
                   ("out_done", out_done, _I32, (P,)), ("status", status, _I32, (1,)), together=(("out_area", "out_box"),))
    _call(_entry("cvlm_mask_thin_sized", host, bits), bits.data_ptr(), bits.numel(), offsets.data_ptr(), dims.data_ptr(), max_iter.data_ptr(), P,
          int(max_words), int(mode), int(steps), workspace.data_ptr(), workspace.numel(), out_bits.data_ptr(), _p(out_area), _p(out_box),
          out_iters.data_ptr(), out_done.data_ptr(), status.data_ptr())


def mask_thin_sized(bits: torch.Tensor, offsets: torch.Tensor, dims: torch.Tensor, max_iter: torch.Tensor, max_words: int, mode: int,
                    steps: int, workspace: torch.Tensor, out_bits: torch.Tensor, out_area: Optional[torch.Tensor],
                    out_box: Optional[torch.Tensor], out_iters: torch.Tensor, out_done: torch.Tensor, status: torch.Tensor) -> None:
    """Each sized plane thinned by Guo & Hall's rule (include/cvlm.h: cvlm_mask_thin_sized): bits flat uint8, byte offsets
    int64 [P + 1], dims int32 [P][2], max_iter int32 [P] in 0 .. 2^30 (0: to the fixed point) -> out_bits (the same layout), out_area
    int32 [P] and out_box int32 [P][4] or both None, out_iters int32 [P] (the iterations that cleared a pixel), out_done int32 [P] (0:
    `steps` ran out), status int32 [1] = 1 if a plane was refused.  mode 0: planes that fit the resident kernel's LDS are thinned there,
    the others in `steps` stepped iterations; mode 1: every plane is stepped.  workspace: uint8, `mask_thin_workspace_bytes`.
    max_words: the largest h * ceil(w / 32) of the call."""
    _mask_thin_sized(False, bits, offsets, dims, max_iter, max_words, mode, steps, workspace, out_bits, out_area, out_box, out_iters,
                     out_done, status)


@functools.wraps(mask_thin_sized, assigned=())        # help() and inspect.signature show the parameter list above
def mask_thin_sized_host(*args, **kw) -> None:
    """`mask_thin_sized` on HOST tensors without a device (cvlm_debug_mask_thin_sized_host: the same word function run sequentially,
    every plane to its fixed point or its max_iter)."""
    _mask_thin_sized(True, *args, **kw)


# ---- Instances: regions of sized planes, the alpha of a region -----------------------------------------------------------------
REGIONS_MAXM = 64                 # rows of the table, and planes a plane is split into (csrc/regions_logic.h: RG_MAXM)


def mask_regions_workspace_bytes(n_bytes: int, P: int, max_words: int) -> int:
    """Bytes of workspace that keep all P planes of one `mask_regions_sized` call in flight (112 per byte of bits, host arithmetic);
    `mask_regions_workspace_bytes(4 * max_words, 1, max_words)`, the largest plane's alone, is the least the entry takes."""
    return _workspace_bytes("cvlm_mask_regions_workspace_bytes", n_bytes, P, max_words)


def _mask_regions_sized(host: bool, bits, offsets, dims, max_words, connectivity, min_area, workspace, n_regions, regions, out_bits, status) -> None:
    """The body of `mask_regions_sized` and of its host twin."""
    P = _sized_planes(bits, offsets, dims)
    _check_tensors(bits, ("regions", regions, _I32, (P, None, 6)), ("workspace", workspace, _U8, (None,)), ("n_regions", n_regions, _I32, (P,)),
                   ("out_bits", out_bits, _U8, (None,)), ("status", status, _I32, (1,)), optional=("workspace",) if host else ())
    M = int(regions.shape[1])
    assert out_bits.numel() == M * bits.numel()
    _call(_entry("cvlm_mask_regions_sized", host, bits), bits.data_ptr(), bits.numel(), offsets.data_ptr(), dims.data_ptr(), P, int(max_words),
          int(connectivity), M, int(min_area), *(() if host else (workspace.data_ptr(), workspace.numel())), n_regions.data_ptr(),
          regions.data_ptr(), out_bits.data_ptr(), status.data_ptr())


def mask_regions_sized(bits: torch.Tensor, offsets: torch.Tensor, dims: torch.Tensor, max_words: int, connectivity: int, min_area: int,
                       workspace: torch.Tensor, n_regions: torch.Tensor, regions: torch.Tensor, out_bits: torch.Tensor,
                       status: torch.Tensor) -> None:
    """Each sized plane split into its connected regions (include/cvlm.h: cvlm_mask_regions_sized): bits flat uint8, byte
    offsets int64 [P + 1], dims int32 [P][2] -> n_regions int32 [P] (the regions of at least max(min_area, 1) pixels), regions int32
    [P][M][6] = (area, x0, y0, x1, y1, seed) of the M largest, out_bits uint8 [M * bits.numel()]: plane (p, m) at byte M * offsets[p] +
    m * (offsets[p + 1] - offsets[p]); status int32 [1] = 1 if a plane was refused.  workspace: uint8, at least the largest plane's
    `mask_regions_workspace_bytes`; less than all planes' makes the entry walk them in rounds.  max_words: the largest h * ceil(w / 32)."""
    _mask_regions_sized(False, bits, offsets, dims, max_words, connectivity, min_area, workspace, n_regions, regions, out_bits, status)


def mask_regions_sized_host(bits: torch.Tensor, offsets: torch.Tensor, dims: torch.Tensor, max_words: int, connectivity: int, min_area: int,
                            n_regions: torch.Tensor, regions: torch.Tensor, out_bits: torch.Tensor, status: torch.Tensor) -> None:
    """`mask_regions_sized` on HOST tensors without a device or a workspace (cvlm_debug_mask_regions_sized_host)."""
    _mask_regions_sized(True, bits, offsets, dims, max_words, connectivity, min_area, None, n_regions, regions, out_bits, status)


def _region_alpha(host: bool, bits, offsets, dims, alpha, src, out, status) -> None:
    """The body of `region_alpha` and of its host twin."""
    Q = _sized_planes(bits, offsets, dims)
    _check_tensors(bits, ("alpha", alpha, _F32, None), ("src", src, _I32, (Q,)), ("out", out, _F32, None), ("status", status, _I32, (1,)))
    assert alpha.dim() in (3, 4) and alpha.shape[-1] == alpha.shape[-2]
    N, R = int(alpha.shape[0]), int(alpha.shape[-1])
    assert alpha.numel() == N * R * R and out.numel() == Q * R * R
    _call(_entry("cvlm_region_alpha", host, bits), bits.data_ptr(), bits.numel(), offsets.data_ptr(), dims.data_ptr(), Q, alpha.data_ptr(), N, R,
          src.data_ptr(), out.data_ptr(), status.data_ptr())


def region_alpha(bits: torch.Tensor, offsets: torch.Tensor, dims: torch.Tensor, alpha: torch.Tensor, src: torch.Tensor, out: torch.Tensor,
                 status: torch.Tensor) -> None:
    """The stage-2 alpha of Q regions (include/cvlm.h: cvlm_region_alpha): out[q] = alpha[src[q]] * the bits of sized plane
    q resized to R x R by `bilinear`'s arithmetic.  alpha f32 [N][R][R] or [N][1][R][R], src int32 [Q] in [0, N), out f32 of Q * R * R
    values; status int32 [1] = 1 if a plane or a src was refused (its out is 0)."""
    _region_alpha(False, bits, offsets, dims, alpha, src, out, status)


@functools.wraps(region_alpha, assigned=())        # help() and inspect.signature show the parameter list above
def region_alpha_host(*args, **kw) -> None:
    """`region_alpha` on HOST tensors without a device (cvlm_debug_region_alpha_host)."""
    _region_alpha(True, *args, **kw)


NMS_MEASURES = {"iou": 0, "min": 1}               # csrc/nms_logic.h: NM_IOU, NM_MIN
NMS_METHODS = {"greedy": 0, "linear": 1, "gaussian": 2}


def mask_nms_inter(bits: torch.Tensor, offsets: torch.Tensor, dims: torch.Tensor, area: torch.Tensor, box: torch.Tensor,
                   group_offsets: torch.Tensor, member: torch.Tensor, pair_offsets: torch.Tensor, inter: torch.Tensor, status: torch.Tensor,
                   host: bool = False) -> None:
    """Intersections of the pairs of each group of sized planes, inside the two boxes alone (include/cvlm.h: cvlm_mask_nms_inter; DESIGN.md
    §30): the sized table of Q planes with area int32 [Q] and box int32 [Q][4], group_offsets int32 [G + 1] into member int32 [Q],
    pair_offsets int64 [G + 1] -> inter int32 [N], group g's triangle at pair_offsets[g], -1 for a refused pair; status int32 [1]: bit 0
    a pair, bit 1 a group was refused.  host=True: the same on HOST tensors without a device (cvlm_debug_mask_nms_inter_host)."""
    Q = _sized_planes(bits, offsets, dims)
    G, N = int(group_offsets.numel()) - 1, int(inter.numel())
    _check_tensors(bits, ("area", area, _I32, (Q,)), ("box", box, _I32, (Q, 4)), ("group_offsets", group_offsets, _I32, (G + 1,)),
                   ("member", member, _I32, (Q,)), ("pair_offsets", pair_offsets, _I64, (G + 1,)), ("inter", inter, _I32, (N,)),
                   ("status", status, _I32, (1,)))
    _call(_entry("cvlm_mask_nms_inter", host, bits), bits.data_ptr(), bits.numel(), offsets.data_ptr(), dims.data_ptr(), area.data_ptr(),
          box.data_ptr(), Q, group_offsets.data_ptr(), member.data_ptr(), pair_offsets.data_ptr(), G, N, _pn(inter), status.data_ptr())


def mask_nms(group_offsets: torch.Tensor, member: torch.Tensor, pair_offsets: torch.Tensor, inter: torch.Tensor, area: torch.Tensor,
             score: torch.Tensor, category: Optional[torch.Tensor], measure: int, method: int, thr: float, sigma: float, order: torch.Tensor,
             keep: torch.Tensor, by: torch.Tensor, decay: torch.Tensor, n_keep: torch.Tensor, status: torch.Tensor, host: bool = False) -> None:
    """Greedy or Matrix NMS of the groups of `mask_nms_inter` (include/cvlm.h: cvlm_mask_nms): area int32, score f32 and
    category int32 (or None) [Q]; measure NMS_MEASURES, method NMS_METHODS; thr and sigma go as doubles -> order int32, keep uint8, by
    int32 and decay f32 [Q], n_keep int32 [G], status int32 [1]: bit 1 a group was refused.  host=True: the same on HOST tensors without
    a device (cvlm_debug_mask_nms_host)."""
    G, N, Q = int(group_offsets.numel()) - 1, int(inter.numel()), int(area.numel())
    _check_tensors(area, ("group_offsets", group_offsets, _I32, (G + 1,)), ("member", member, _I32, (Q,)), ("pair_offsets", pair_offsets, _I64, (G + 1,)),
                   ("inter", inter, _I32, (N,)), ("area", area, _I32, (Q,)), ("score", score, _F32, (Q,)), ("category", category, _I32, (Q,)),
                   ("order", order, _I32, (Q,)), ("keep", keep, _U8, (Q,)), ("by", by, _I32, (Q,)), ("decay", decay, _F32, (Q,)),
                   ("n_keep", n_keep, _I32, (G,)), ("status", status, _I32, (1,)), optional=("category",))
    params = (C.c_double * 2)(float(thr), float(sigma))               # host memory: the entry reads it before it returns
    _call(_entry("cvlm_mask_nms", host, area), group_offsets.data_ptr(), member.data_ptr(), pair_offsets.data_ptr(), G, _pn(inter), N,
          area.data_ptr(), score.data_ptr(), _p(category), Q, int(measure), int(method), C.addressof(params), order.data_ptr(), keep.data_ptr(),
          by.data_ptr(), decay.data_ptr(), n_keep.data_ptr(), status.data_ptr())


RENDER_KINDS = {"bits": 0, "levels": 1, "labels": 2}      # csrc/render_logic.h: RD_BITS, RD_LEVELS, RD_LABELS
RENDER_EDGES, RENDER_INVERT = 1, 2                        # flags: RD_EDGES (labels), RD_INVERT (bits)


def render(img: torch.Tensor, img_offsets: torch.Tensor, dims: torch.Tensor, max_pixels: int, layer_offsets: torch.Tensor,
           layers: Optional[torch.Tensor], bits: Optional[torch.Tensor], levels: Optional[torch.Tensor], labels: Optional[torch.Tensor],
           rgb: torch.Tensor, alpha: torch.Tensor, out: torch.Tensor, status: torch.Tensor, host: bool = False) -> None:
    """Layers painted over B interleaved 3-channel uint8 images of their own sizes (include/cvlm.h: cvlm_render): img and
    out flat uint8 of equal length (out may BE img: in place), img_offsets int64 [B + 1] in bytes, dims int32 [B][2], layer_offsets int32
    [B + 1] into layers int64 [L][4] = (kind | flags << 8, src, first, rows) (None: L = 0); the sources bits uint8, levels uint8 and
    labels int32, each flat or None; the table rgb uint8 [T][3] and alpha f32 [T]; status int32 [1]: bit 0 an image was refused, bit 1
    a layer skipped, bit 2 a table row with an alpha that paints nothing was selected.  host=True: the same on HOST tensors without a
    device (cvlm_debug_render_host)."""
    B, T = int(dims.shape[0]), int(alpha.numel())
    L = 0 if layers is None else int(layers.shape[0])
    _check_tensors(img, ("img", img, _U8, (None,)), ("out", out, _U8, (img.numel(),)), ("img_offsets", img_offsets, _I64, (B + 1,)),
                   ("dims", dims, _I32, (B, 2)), ("layer_offsets", layer_offsets, _I32, (B + 1,)), ("rgb", rgb, _U8, (T, 3)), ("alpha", alpha, _F32, (T,)),
                   ("status", status, _I32, (1,)), ("layers", layers, _I64, (L, 4)), ("bits", bits, _U8, (None,)), ("levels", levels, _U8, (None,)),
                   ("labels", labels, _I32, (None,)), optional=("layers", "bits", "levels", "labels"))
    n = lambda t: 0 if t is None else int(t.numel())
    _call(_entry("cvlm_render", host, img), img.data_ptr(), img.numel(), img_offsets.data_ptr(), dims.data_ptr(), B, int(max_pixels),
          layer_offsets.data_ptr(), _p(layers) if L else None, L, _p(bits), n(bits), _p(levels), n(levels), _p(labels), n(labels), rgb.data_ptr(),
          alpha.data_ptr(), T, out.data_ptr(), status.data_ptr())


# ---- label maps: the tensors below live on the device for the cvlm_label_* entries and on the host for `host=True` ----
def _label_state(score, winner, segment, areas, segment_id, n_segments, status, B: int, K: int, without=()) -> int:
    """The check of the state and outputs of the label entries (`without`: what an entry does not take) -> n_pix."""
    n_pix = winner.numel()
    _check_tensors(winner, ("score", score, _F32, (n_pix,)), ("winner", winner, _I16, (n_pix,)), ("segment", segment, _I16, (n_pix,)),
                   ("areas", areas, _I32, (3, B * K)), ("segment_id", segment_id, _I32, (B * K,)), ("n_segments", n_segments, _I32, (B,)),
                   ("status", status, _I32, (1,)), optional=without)
    return n_pix


def _label_tables(dims, pix_offsets, B: int, like: torch.Tensor) -> None:
    _check_tensors(like, ("dims", dims, _I32, (B, 2)), ("pix_offsets", pix_offsets, _I64, (B + 1,)))


def label_init(score, winner, segment, areas, segment_id, n_segments, status, B: int, K: int, host: bool = False) -> None:
    """The fill of a label-map state (include/cvlm.h: cvlm_label_init): score f32 [n_pix] = 0, winner / segment int16 [n_pix] = -1,
    areas int32 [3][B * K] = segment_id int32 [B * K] = n_segments int32 [B] = 0, status int32 [1] = 0."""
    n_pix = _label_state(score, winner, segment, areas, segment_id, n_segments, status, B, K)
    _call(_entry("cvlm_label_init", host, score), score.data_ptr(), winner.data_ptr(), segment.data_ptr(), n_pix, areas.data_ptr(),
          segment_id.data_ptr(), B, K, n_segments.data_ptr(), status.data_ptr())


def label_accumulate(planes: torch.Tensor, p0: int, B: int, K: int, dims, pix_offsets, weights, level: int, score, winner, segment,
                     max_pixels: int, areas, status, host: bool = False) -> None:
    """planes f32 [n][Hs][Ws] = the planes p0 .. p0 + n - 1 of B * K, offered in increasing k to the pixels of their images
    (cvlm_label_accumulate): dims int32 [B][2], pix_offsets int64 [B + 1] in pixels, weights f32 [B * K] or None."""
    n, Hs, Ws = planes.shape
    assert isinstance(level, int)
    n_pix = _label_state(score, winner, segment, areas, None, None, status, B, K, without=("segment_id", "n_segments"))
    _label_tables(dims, pix_offsets, B, score)
    _check_tensors(score, ("planes", planes, _F32, (n, Hs, Ws)), ("weights", weights, _F32, None), optional=("weights",))
    assert weights is None or weights.numel() == B * K
    _call(_entry("cvlm_label_accumulate", host, score), planes.data_ptr(), p0, p0 + n, Hs, Ws, B, K, dims.data_ptr(), pix_offsets.data_ptr(),
          _p(weights), level, score.data_ptr(), winner.data_ptr(), segment.data_ptr(), n_pix, int(max_pixels), areas.data_ptr(),
          status.data_ptr())


def label_finish(B: int, K: int, dims, pix_offsets, overlap_threshold: float, winner, segment, max_pixels: int, areas, segment_id,
                 n_segments, status, host: bool = False) -> None:
    """won_area, kept_area, kept / segment_id / n_segments and the final `segment` map from the state (cvlm_label_finish); the
    threshold is handed over as one host double."""
    n_pix = _label_state(None, winner, segment, areas, segment_id, n_segments, status, B, K, without=("score",))
    _label_tables(dims, pix_offsets, B, winner)
    thr = C.c_double(overlap_threshold)
    _call(_entry("cvlm_label_finish", host, winner), B, K, dims.data_ptr(), pix_offsets.data_ptr(), C.addressof(thr), winner.data_ptr(),
          segment.data_ptr(), n_pix, int(max_pixels), areas.data_ptr(), segment_id.data_ptr(), n_segments.data_ptr(), status.data_ptr())


def label_lookup(map_: torch.Tensor, B: int, K: int, dims, pix_offsets, max_pixels: int, table: torch.Tensor, void: int, out: torch.Tensor,
                 status: torch.Tensor, host: bool = False) -> None:
    """out int32 [n_pix] = map < 0 ? void : table[b * K + map] for the pixels of every image (cvlm_label_lookup)."""
    n_pix = map_.numel()
    _check_tensors(map_, ("map_", map_, _I16, (n_pix,)), ("table", table, _I32, None), ("out", out, _I32, (n_pix,)), ("status", status, _I32, (1,)))
    assert table.numel() == B * K
    _label_tables(dims, pix_offsets, B, map_)
    _call(_entry("cvlm_label_lookup", host, map_), map_.data_ptr(), B, K, dims.data_ptr(), pix_offsets.data_ptr(), n_pix, int(max_pixels),
          table.data_ptr(), int(void), out.data_ptr(), status.data_ptr())


def label_iou_hist(pred: torch.Tensor, gt: torch.Tensor, num_classes: int, ignore_index: int, reduce_zero_label: bool, zero_first: bool,
                   totals: torch.Tensor, host: bool = False) -> None:
    """totals int64 [3][C] += (area_intersect, area_pred_label, area_label) of pred int32 [n] against gt int32 or uint8 [n]
    (cvlm_label_iou_hist: mmseg's intersect_and_union)."""
    gt_u8 = gt.dtype == _U8
    _check_tensors(pred, ("pred", pred, _I32, (None,)), ("gt", gt, _U8 if gt_u8 else _I32, tuple(pred.shape)),
                   ("totals", totals, _I64, (3, num_classes)))
    _call(_entry("cvlm_label_iou_hist", host, pred), pred.data_ptr(), gt.data_ptr(), int(gt_u8), pred.numel(), num_classes, int(ignore_index),
          int(bool(reduce_zero_label)), int(bool(zero_first)), totals.data_ptr())


# ---- panoptic quality: device tensors for the cvlm_pan_* entries, host tensors for `host=True` ------------------------------
def pan_lds_cells() -> int:
    """The G * S up to which cvlm_pan_pair_hist keeps an image's table in LDS (csrc/panoptic_logic.h: pn_lds_cells)."""
    return int(load().cvlm_debug_pan_lds_cells())


def pan_remap(raw: torch.Tensor, B: int, dims, pix_offsets, max_pixels: int, keys, vals, table_offsets, out, unknown, status,
              host: bool = False) -> None:
    """out int32 [n_pix] = the dense index of each pixel's raw id -- raw uint8 [n_pix][3] (rgb2id) or int32 [n_pix] -- looked up in image
    b's slice table_offsets[b] .. table_offsets[b + 1] of keys (ascending) / vals; unknown int32 [B] = the pixels whose non-zero id the
    table does not hold (cvlm_pan_remap)."""
    rgb = raw.dtype == _U8
    n_pix, n_keys = out.numel(), keys.numel()
    _check_tensors(raw, ("raw", raw, _U8 if rgb else _I32, (n_pix, 3) if rgb else (n_pix,)), ("keys", keys, _I32, (n_keys,)),
                   ("vals", vals, _I32, (n_keys,)), ("table_offsets", table_offsets, _I64, (B + 1,)), ("out", out, _I32, (n_pix,)),
                   ("unknown", unknown, _I32, (B,)), ("status", status, _I32, (1,)))
    _label_tables(dims, pix_offsets, B, raw)
    _call(_entry("cvlm_pan_remap", host, raw), raw.data_ptr(), int(rgb), B, dims.data_ptr(), pix_offsets.data_ptr(), n_pix, int(max_pixels),
          keys.data_ptr(), vals.data_ptr(), table_offsets.data_ptr(), n_keys, out.data_ptr(), unknown.data_ptr(), status.data_ptr())


def pan_pair_hist(pred, gt, B: int, G: int, S: int, dims, pix_offsets, max_pixels: int, zero_first: bool, inter, status,
                  host: bool = False) -> None:
    """inter int32 [B][G][S] += the pixels of image b with gt = g and pred = s, both int32 [n_pix] (cvlm_pan_pair_hist)."""
    n_pix = pred.numel()
    _check_tensors(pred, ("pred", pred, _I32, (n_pix,)), ("gt", gt, _I32, (n_pix,)), ("inter", inter, _I32, (B, G, S)), ("status", status, _I32, (1,)))
    _label_tables(dims, pix_offsets, B, pred)
    _call(_entry("cvlm_pan_pair_hist", host, pred), pred.data_ptr(), gt.data_ptr(), B, G, S, dims.data_ptr(), pix_offsets.data_ptr(), n_pix,
          int(max_pixels), int(bool(zero_first)), inter.data_ptr(), status.data_ptr())


def pan_match(inter, pred_cat, gt_cat, gt_crowd, num_classes: int, pred_match, pred_iou, gt_match, pred_area, gt_area,
              host: bool = False) -> None:
    """Steps 2 to 4 of DESIGN.md §24 per image from inter int32 [B][G][S], pred_cat int32 [B][S], gt_cat int32 [B][G] and gt_crowd uint8
    [B][G] -> pred_match / pred_area int32 [B][S], pred_iou f64 [B][S], gt_match / gt_area int32 [B][G] (cvlm_pan_match)."""
    assert inter.dim() == 3
    B, G, S = inter.shape
    _check_tensors(inter, ("inter", inter, _I32, (B, G, S)), ("pred_cat", pred_cat, _I32, (B, S)), ("gt_cat", gt_cat, _I32, (B, G)),
                   ("gt_crowd", gt_crowd, _U8, (B, G)), ("pred_match", pred_match, _I32, (B, S)), ("pred_iou", pred_iou, _F64, (B, S)),
                   ("gt_match", gt_match, _I32, (B, G)), ("pred_area", pred_area, _I32, (B, S)), ("gt_area", gt_area, _I32, (B, G)))
    _call(_entry("cvlm_pan_match", host, inter), inter.data_ptr(), B, G, S, pred_cat.data_ptr(), gt_cat.data_ptr(), gt_crowd.data_ptr(),
          int(num_classes), pred_match.data_ptr(), pred_iou.data_ptr(), gt_match.data_ptr(), pred_area.data_ptr(), gt_area.data_ptr())


def pan_accumulate(pred_cat, gt_cat, pred_match, pred_iou, gt_match, num_classes: int, zero_first: bool, counts, iou_sum,
                   host: bool = False) -> None:
    """counts int64 [3][C] (tp, fp, fn) and iou_sum f64 [C] += what cvlm_pan_match stored for a batch (cvlm_pan_accumulate)."""
    B, S = pred_cat.shape
    G = gt_cat.shape[1]
    _check_tensors(pred_cat, ("pred_cat", pred_cat, _I32, (B, S)), ("gt_cat", gt_cat, _I32, (B, G)), ("pred_match", pred_match, _I32, (B, S)),
                   ("pred_iou", pred_iou, _F64, (B, S)), ("gt_match", gt_match, _I32, (B, G)), ("counts", counts, _I64, (3, num_classes)),
                   ("iou_sum", iou_sum, _F64, (num_classes,)))
    _call(_entry("cvlm_pan_accumulate", host, pred_cat), B, G, S, pred_cat.data_ptr(), gt_cat.data_ptr(), pred_match.data_ptr(),
          pred_iou.data_ptr(), gt_match.data_ptr(), int(num_classes), int(bool(zero_first)), counts.data_ptr(), iou_sum.data_ptr())


def topk_accumulate(scores: torch.Tensor, labels: torch.Tensor, pred: Optional[torch.Tensor], counters: torch.Tensor) -> None:
    """scores f32 [B][C], labels int32 [B] -> pred int32 [B]; counters int32 [3] += (top-1, top-5, rows)."""
    B, Cc = scores.shape
    _check_tensors(scores, ("scores", scores, _F32, (B, Cc)), ("labels", labels, _I32, None), ("counters", counters, _I32, None))
    assert labels.numel() == B and counters.numel() == 3
    _call("cvlm_topk_accumulate", scores.data_ptr(), labels.data_ptr(), B, Cc, _p(pred), counters.data_ptr())


def mask_wfm_workspace_bytes(N: int, h: int, w: int) -> int:
    return N * h * w * 16 + N * ((h * w + 255) // 256) * 24 + N * 8


def mask_wfm(pre: torch.Tensor, gt: torch.Tensor, hist: torch.Tensor, gauss49: torch.Tensor, workspace: torch.Tensor,
             out3: torch.Tensor) -> None:
    """pre/gt uint8 [N][h][w], hist int32 [N][4][2][256] (from mask_joint_hist), gauss49 float64 [49],
    workspace uint8 [>= mask_wfm_workspace_bytes], out3 float64 [N][3]."""
    N, h, w = pre.shape
    assert pre.dtype == torch.uint8 and gt.dtype == torch.uint8 and tuple(gt.shape) == (N, h, w)
    assert hist.dtype == torch.int32 and gauss49.dtype == torch.float64 and gauss49.numel() == 49
    assert out3.dtype == torch.float64 and tuple(out3.shape) == (N, 3) and workspace.numel() * workspace.element_size() >= mask_wfm_workspace_bytes(N, h, w)
    assert pre.is_contiguous() and gt.is_contiguous() and hist.is_contiguous()
    _call("cvlm_mask_wfm", pre.data_ptr(), gt.data_ptr(), N, h, w, hist.data_ptr(), gauss49.data_ptr(), workspace.data_ptr(), out3.data_ptr())


def prob_workspace_bytes(N: int, h: int, w: int) -> int:
    """workspace of the three cvlm_prob_* calls (include/cvlm.h, ABI 8)"""
    return max(mask_wfm_workspace_bytes(N, h, w), N * 8192)


def prob_quantise(prob: torch.Tensor, minmax: torch.Tensor, q: torch.Tensor, workspace: torch.Tensor) -> None:
    """prob f32 [N][h][w] -> minmax f32 [N][2], q uint8 [N][h][w] (utils.calc_cod's `_prepare_data` + the E-measure's levels)."""
    N, h, w = prob.shape
    assert prob.dtype == torch.float32 and prob.is_contiguous() and minmax.dtype == torch.float32 and tuple(minmax.shape) == (N, 2)
    assert q.dtype == torch.uint8 and tuple(q.shape) == (N, h, w) and q.is_contiguous() and workspace.numel() >= prob_workspace_bytes(N, h, w)
    _call("cvlm_prob_quantise", prob.data_ptr(), N, h, w, minmax.data_ptr(), q.data_ptr(), workspace.data_ptr())


def prob_moments(prob: torch.Tensor, gt: torch.Tensor, minmax: torch.Tensor, stats: torch.Tensor, workspace: torch.Tensor,
                 out: torch.Tensor) -> None:
    """-> out f64 [N][4][2][2]: (sum pn, sum pn^2) per S-measure quadrant and ground-truth class; stats from mask_joint_hist."""
    N, h, w = prob.shape
    assert gt.dtype == torch.uint8 and tuple(gt.shape) == (N, h, w) and gt.is_contiguous() and stats.dtype == torch.int64
    assert out.dtype == torch.float64 and tuple(out.shape) == (N, 4, 2, 2) and workspace.numel() >= prob_workspace_bytes(N, h, w)
    _call("cvlm_prob_moments", prob.data_ptr(), gt.data_ptr(), N, h, w, minmax.data_ptr(), stats.data_ptr(), workspace.data_ptr(), out.data_ptr())


def prob_wfm(prob: torch.Tensor, gt: torch.Tensor, minmax: torch.Tensor, gauss49: torch.Tensor, workspace: torch.Tensor,
             out3: torch.Tensor) -> None:
    N, h, w = prob.shape
    assert out3.dtype == torch.float64 and tuple(out3.shape) == (N, 3) and gauss49.dtype == torch.float64 and gauss49.numel() == 49
    assert workspace.numel() >= prob_workspace_bytes(N, h, w)
    _call("cvlm_prob_wfm", prob.data_ptr(), gt.data_ptr(), N, h, w, minmax.data_ptr(), gauss49.data_ptr(), workspace.data_ptr(), out3.data_ptr())
