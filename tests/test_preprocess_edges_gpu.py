"""N1 at the edges (csrc/preprocess.hip): every kernel and branch cvlm_resample_u8 and cvlm_u8_to_tensor choose between, at the shapes,
strides and pointer offsets of tests/ends_cases.py, bit for bit against oracle/preprocess_oracle.py (pinned to Pillow) and, for whole
resizes, against Pillow itself.  Every output lives inside a larger prefilled buffer whose other bytes must stay untouched, and every
test checks the restated dispatch rule on the pointers it really passes, so a case cannot drift off the path it names."""
import numpy as np
import pytest
import torch

import ends_cases as EC
from oracle import preprocess_oracle as P

pytestmark = pytest.mark.gpu
GUARD = 64


def _embed(nbytes: int, off: int):
    """a prefilled uint8 device buffer and the byte range [start, start + nbytes) inside it, `off` bytes past a 16-byte boundary"""
    buf = torch.full((GUARD + 16 + nbytes + GUARD,), EC.SENTINEL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    start = GUARD + off
    return buf, start


def _put(arr: np.ndarray, off: int) -> torch.Tensor:
    buf, start = _embed(arr.nbytes, off)
    view = buf[start:start + arr.nbytes].view(arr.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)).cuda())
    return view


def _untouched(buf: torch.Tensor, start: int, nbytes: int) -> bool:
    return bool((buf[:start] == EC.SENTINEL).all()) and bool((buf[start + nbytes:] == EC.SENTINEL).all())


@pytest.mark.parametrize("c", EC.RESAMPLE_CASES, ids=lambda c: c.id)
def test_resample_one_axis_bit_exact(c):
    from camouflaged_vlm_amd import hip
    img = EC.resample_input(c)
    src = _put(img, c.src_off)
    nbytes = int(np.prod(c.out_shape))
    for filt in c.filters:
        b, k = EC.resample_tables(c, filt)
        buf, start = _embed(nbytes, c.dst_off)
        dst = buf[start:start + nbytes].view(c.out_shape)
        assert EC.resample_path(c.N, c.H, c.W, c.C, c.n_out, c.axis, src.data_ptr(), dst.data_ptr()) == c.path
        hip.resample_u8(src, torch.from_numpy(b).cuda(), torch.from_numpy(k).cuda(), c.n_out, c.axis, dst)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        want = np.stack([P._pass(img[n], b, k, c.axis) for n in range(c.N)])
        assert np.array_equal(got, want), (c.id, filt, int((got != want).sum()))
        assert _untouched(buf, start, nbytes), (c.id, filt)
        if c.pattern == "blocks":
            assert (got == 0).any() and (got == 255).any()
    assert torch.equal(src.cpu(), torch.from_numpy(img))


def _pillow_resize(a: np.ndarray, oh: int, ow: int, filt: str):
    """PIL.Image.resize of an HWC array, channel by channel as mode L (Pillow premultiplies RGBA); C = 3 also as one RGB image"""
    from PIL import Image
    f = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "nearest": Image.NEAREST}[filt]
    out = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(a[:, :, ch])).resize((ow, oh), f)) for ch in range(a.shape[2])], axis=2)
    if a.shape[2] == 3:
        assert np.array_equal(out, np.asarray(Image.fromarray(a).resize((ow, oh), f)))
    return out


@pytest.mark.parametrize("size", EC.RESIZE_CASES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-to-{s[1][0]}x{s[1][1]}")
def test_whole_resize_equals_oracle_and_pillow(size):
    from camouflaged_vlm_amd.preprocess import GpuPreprocess, nearest_indices
    (h, w), (oh, ow) = size
    pre = GpuPreprocess(64, 56)
    rng = np.random.default_rng(h * 10007 + w)
    for C in EC.RESIZE_CHANNELS:
        a = rng.integers(0, 256, (h, w, C), dtype=np.uint8)
        dev = torch.from_numpy(a).cuda()[None]
        for filt in ("bilinear", "bicubic", "nearest"):
            got = pre.resize(dev, oh, ow, filt)[0].cpu().numpy()
            want = a[nearest_indices(h, oh)][:, nearest_indices(w, ow)] if filt == "nearest" else P.resize_u8(a, oh, ow, filt)
            assert np.array_equal(got, want), (size, C, filt)
            try:
                import PIL.Image  # noqa: F401
            except ImportError:
                continue
            assert np.array_equal(got, _pillow_resize(a, oh, ow, filt)), (size, C, filt, "Pillow")


@pytest.mark.parametrize("c", EC.TENSOR_CASES, ids=lambda c: c.id)
def test_to_tensor_normalize_crop_exact(c):
    from camouflaged_vlm_amd import hip
    img, mean, std = EC.tensor_input(c)
    src = _put(img, c.src_off)
    nbytes = c.N * c.C * c.ch * c.cw * 4
    buf, start = _embed(nbytes, c.dst_off)
    dst = buf[start:start + nbytes].view(torch.float32).view(c.N, c.C, c.ch, c.cw)
    path, word, byte = EC.tensor_path(c.N, c.H, c.W, c.C, c.top, c.left, c.ch, c.cw, src.data_ptr(), dst.data_ptr())
    assert path == c.path and (not c.both_branches or (word > 0 and byte > 0))
    hip.u8_to_tensor(src, c.top, c.left, c.ch, c.cw, torch.from_numpy(mean).cuda(), torch.from_numpy(std).cuda(), dst)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    want = EC.tensor_reference(c)
    assert got.dtype == want.dtype == np.float32 and np.array_equal(got, want), (c.id, float(np.abs(got - want).max()))
    assert _untouched(buf, start, nbytes), c.id


def test_preprocess_entries_refuse_bad_arguments():
    """CVLM_E_BADARG (-1) before anything is launched: the destination keeps its prefill"""
    from camouflaged_vlm_amd import hip
    src = torch.zeros((1, 4, 6, 3), dtype=torch.uint8, device="cuda")
    mean = torch.zeros(3, device="cuda")
    out = torch.full((1, 3, 4, 6), 7.0, device="cuda")
    for top, left, ch, cw in ((1, 0, 4, 6), (0, 1, 4, 6), (-1, 0, 2, 2), (0, -1, 2, 2), (3, 0, 2, 2), (0, 5, 2, 2)):
        with pytest.raises(RuntimeError, match="cvlm_u8_to_tensor failed with code -1$"):
            hip.u8_to_tensor(src, top, left, ch, cw, mean, mean, out)
    for args in ((None, 1, 4, 6, 3, 0, 0, 4, 6, mean.data_ptr(), mean.data_ptr(), out.data_ptr()),
                 (src.data_ptr(), 1, 4, 6, 3, 0, 0, 4, 6, None, mean.data_ptr(), out.data_ptr()),
                 (src.data_ptr(), 1, 4, 6, 3, 0, 0, 4, 6, mean.data_ptr(), None, out.data_ptr()),
                 (src.data_ptr(), 1, 4, 6, 3, 0, 0, 4, 6, mean.data_ptr(), mean.data_ptr(), None)):
        with pytest.raises(RuntimeError, match="code -1$"):
            hip._call("cvlm_u8_to_tensor", *args)
    b = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
    k = torch.zeros((5, 3), dtype=torch.int32, device="cuda")
    dst = torch.full((1, 4, 5, 3), EC.SENTINEL, dtype=torch.uint8, device="cuda")
    s, d, bp, kp = src.data_ptr(), dst.data_ptr(), b.data_ptr(), k.data_ptr()
    for args in ((None, 1, 4, 6, 3, bp, kp, 3, 5, 1, d), (s, 1, 4, 6, 3, None, kp, 3, 5, 1, d), (s, 1, 4, 6, 3, bp, None, 3, 5, 1, d),
                 (s, 1, 4, 6, 3, bp, kp, 3, 5, 1, None), (s, 0, 4, 6, 3, bp, kp, 3, 5, 1, d), (s, 1, 0, 6, 3, bp, kp, 3, 5, 1, d),
                 (s, 1, 4, 0, 3, bp, kp, 3, 5, 1, d), (s, 1, 4, 6, 0, bp, kp, 3, 5, 1, d), (s, 1, 4, 6, 3, bp, kp, 0, 5, 1, d),
                 (s, 1, 4, 6, 3, bp, kp, 3, 0, 1, d), (s, 1, 4, 6, 3, bp, kp, 3, 5, 2, d), (s, 1, 4, 6, 3, bp, kp, 3, 5, -1, d)):
        with pytest.raises(RuntimeError, match="cvlm_resample_u8 failed with code -1$"):
            hip._call("cvlm_resample_u8", *args)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((dst == EC.SENTINEL).all())


@pytest.mark.parametrize("hw", EC.PIPELINE_IMAGES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_clip_and_sam_input_on_portrait_and_landscape(hw):
    """the whole N1 step at a small model size: the resized side is odd (83), so rows of the centre crop alternate between the two
    branches of the four-pixel kernel, and the crop starts at column 14 (landscape) or row 14 (portrait); a batch of two"""
    from camouflaged_vlm_amd.preprocess import GpuPreprocess
    S, R = EC.PIPELINE_SIZES
    pre = GpuPreprocess(S, R)
    rng = np.random.default_rng(hw[0])
    imgs = rng.integers(0, 256, (2,) + hw + (3,), dtype=np.uint8)
    dev = torch.from_numpy(imgs).cuda()
    clip, sam = pre.clip_input(dev).cpu().numpy(), pre.sam_input(dev).cpu().numpy()
    for n in range(2):
        assert np.array_equal(clip[n], P.clip_input(imgs[n], R)), (hw, n)
        assert np.array_equal(sam[n], P.sam_input(imgs[n], S)), (hw, n)
    assert np.array_equal(pre.clip_input(dev[1]).cpu().numpy()[0], clip[1])
