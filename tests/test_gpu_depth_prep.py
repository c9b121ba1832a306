"""-m gpu: the depth-crop resampler (ibl_depth_prep_kernel, csrc/dator.hip) called directly through `ibl_preprocess_depth`, on batches of
differently sized crops (the int64 offsets), against references that share no code with the product:

  layout  a numpy im2col (tests/dator_head_cases.im2col), not the product's `patches_from_pixels`; once with patch_k_pad = 768 and once
          with 800, where columns 768 - 799 must be zero in every row (the zero-fill branch)
  value   taps and weights from the kernel's documented fp32 coordinate rule (oracle.dator_oracle.resize_coords, held to the float64
          rule by tests/test_dator_head_model.py), interpolation, clip and normalisation in float64:
              |got - ref| <= 2^-11 |ref| + 2^-18   at every element
          (half an fp16 step, plus two dozen fp32 roundings of 2^-24 at |d| <= 70 scaled by 2 / 50 = 1.6e-6, doubled)
  bits    at (256, 128) every weight is 0 and at (512, 256) every weight is 0.5 (inputs on a 2^-8 grid: the 2 x 2 mean is exact): the
          output equals numpy float32 arithmetic bit for bit

Shapes: single rows / columns / pixels, the exact output size and one off it on either side, exact 2x, a strong down-sample, and the
three of test_gpu_dator.py.  Contents: a smooth surface, the same with 10 % holes (0), and uniform values in [-5, 70] that reach past
both ends of the 0 - 50 m clip."""
import numpy as np
import pytest
import torch

from oracle import dator_oracle as do
from tests import dator_head_cases as hc

pytestmark = pytest.mark.gpu

OUT_H, OUT_W, PATCH = 256, 128, 16
DMIN, DMAX = 0.0, 50.0
NAN16 = 0x7E00


def run_kernel(crops, kpad):
    """-> uint16 bit patterns [len(crops)][128][kpad]; the output starts as fp16 NaN, so an element the kernel leaves out shows"""
    from ibloc_amd import _lib
    sizes = np.array([c.shape for c in crops], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(sizes[:, 0].astype(np.int64) * sizes[:, 1])]).astype(np.int64)
    flat = torch.from_numpy(np.concatenate([c.reshape(-1) for c in crops])).cuda()
    d_sizes, d_offs = torch.from_numpy(sizes).cuda(), torch.from_numpy(offs[:-1].copy()).cuda()
    rows = len(crops) * (OUT_H // PATCH) * (OUT_W // PATCH)
    patches = torch.full((rows, kpad), NAN16, dtype=torch.int16, device="cuda")
    st = _lib.lib.ibl_preprocess_depth(flat.data_ptr(), d_offs.data_ptr(), d_sizes.data_ptr(), len(crops), OUT_H, OUT_W, PATCH, kpad,
                                       DMIN, DMAX, patches.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(st, "ibl_preprocess_depth")
    return patches.cpu().numpy().view(np.uint16).reshape(len(crops), -1, kpad)


@pytest.fixture(scope="module")
def batch():
    """all shapes x all contents in one batch (36 crops of 12 sizes), and the float64 reference image of each, computed once"""
    crops = [hc.depth_crop(s, c) for c in hc.DEPTH_CONTENTS for s in hc.DEPTH_SHAPES]
    tags = [(s, c) for c in hc.DEPTH_CONTENTS for s in hc.DEPTH_SHAPES]
    refs = [do.preprocess_depth_f64(d, DMIN, DMAX, OUT_H, OUT_W) for d in crops]
    return crops, tags, refs


@pytest.mark.parametrize("kpad", [768, 800])
def test_layout_and_value_on_every_shape_and_content(batch, kpad):
    crops, tags, refs = batch
    bits = run_kernel(crops, kpad)
    got = bits.view(np.float16).astype(np.float64)
    missed = []
    for i, (tag, ref) in enumerate(zip(tags, refs)):
        exp = hc.im2col(ref, PATCH, kpad)
        assert np.isfinite(got[i]).all(), f"{tag}: elements left unwritten or not finite"
        assert not bits[i][:, 3 * PATCH * PATCH:].any(), f"{tag}: columns past 3 * patch^2 are not zero"
        k = 3 * PATCH * PATCH                                   # the columns past it are held to exactly zero above
        gap = np.abs(got[i][:, :k] - exp[:, :k])
        tol = 2.0 ** -11 * np.abs(exp[:, :k]) + 2.0 ** -18
        over = gap - tol
        print(f"[depth prep] kpad {kpad} {str(tag[0]):11s} {tag[1]:8s} largest |got - ref| {gap.max():.3e}, largest excess over the bound "
              f"{over.max():+.3e}; ref in [{ref.min():+.3f}, {ref.max():+.3f}]")
        if over.max() > 0:
            missed.append((tag, float(gap.max()), float(over.max()), np.unravel_index(int(over.argmax()), over.shape)))
    assert not missed, missed
    # the contents do reach what they are there for
    uni = [r for (s, c), r in zip(tags, refs) if c == "uniform" and s[0] * s[1] > 30]
    assert all(r.min() == -1.0 and r.max() == 1.0 for r in uni)
    hole = [c for (s, k), c in zip(tags, crops) if k == "holes" and s[0] * s[1] > 100]
    assert all((c == 0).any() for c in hole)


def test_bit_exact_at_weights_zero_and_one_half():
    f32 = np.float32

    def norm16(d):
        r = np.clip(d.astype(np.float32), f32(DMIN), f32(DMAX))
        r = (r - f32(DMIN)) / f32(DMAX - DMIN)
        return ((r - f32(0.5)) / f32(0.5)).astype(np.float16)

    same = [hc.depth_crop((OUT_H, OUT_W), c) for c in hc.DEPTH_CONTENTS]
    rng = np.random.default_rng(12)
    half = (rng.integers(0, 50 * 256, size=(2 * OUT_H, 2 * OUT_W)).astype(np.float32) / f32(256))          # multiples of 2^-8 in [0, 50)
    for n, o in ((OUT_H, OUT_H), (OUT_W, OUT_W)):
        assert not do.resize_coords(o, n)[2].any()
        assert np.all(do.resize_coords(o, 2 * n)[2] == 0.5)
    bits = run_kernel(same + [half], 768)
    for i, d in enumerate(same):
        exp = hc.im2col(norm16(d), PATCH, 768).view(np.uint16)
        assert np.array_equal(bits[i], exp), f"(256, 128) {hc.DEPTH_CONTENTS[i]}: {(bits[i] != exp).sum()} elements differ in bits"
    mean = (half[0::2, 0::2] + half[0::2, 1::2] + half[1::2, 0::2] + half[1::2, 1::2]) * f32(0.25)         # exact in fp32
    assert np.array_equal(mean.astype(np.float64), (half.astype(np.float64).reshape(OUT_H, 2, OUT_W, 2).sum((1, 3)) / 4))
    exp = hc.im2col(norm16(mean), PATCH, 768).view(np.uint16)
    assert np.array_equal(bits[3], exp), f"(512, 256): {(bits[3] != exp).sum()} elements differ in bits"
