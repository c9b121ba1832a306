"""CPU: the cases of tests/dator_head_cases.py do what their table says, shown with the oracle alone (oracle.dator_oracle.head_stages
in fp64 and fp32), the staged restatement agrees with the pinned `head_forward`, the head's workspace layout query is consistent with
its size query, and the fp32 coordinate rule of the depth resize is the float64 rule on every crop shape of the depth test."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import dator_oracle as do
from tests import dator_head_cases as hc

B = 2


@pytest.fixture(scope="module")
def runs():
    out = {}
    rt, dt = hc.tokens(B)
    for name in hc.CASES:
        hw = hc.case_weights(name)
        out[name] = (hw, rt, dt, do.head_stages(hw, rt, dt, torch.float64), do.head_stages(hw, rt, dt, torch.float32))
    return out


@pytest.mark.parametrize("name", hc.CASES)
def test_every_intermediate_is_finite_and_shaped_like_the_taps(runs, name):
    s64 = runs[name][3]
    R = B * 128
    shapes = {"gl": (B, 128), "lp": (R, 128), "cat": (R, 256), "h1": (R, 128), "h2": (R, 32), "h3": (R, 8), "h4": (R, 2), "rgb_f": (B, 128),
              "depth_f": (B, 128), "q_r": (R, 128), "v_r": (R, 128), "q_d": (R, 128), "v_d": (R, 128), "fr": (R, 128), "fd": (R, 128),
              "out": (B, 128)}
    for op in hc.ATTN_OPS:
        shapes.update({op + ".sel": (R, 48), op + ".aw": (R, 24), op + ".aw_logits": (R, 24), op + ".samp": (R, 128), op + ".feat": (R, 128)})
    for k, shp in shapes.items():
        assert tuple(s64[k].shape) == shp, k
    for k, v in s64.items():
        assert v.dtype == torch.float64 and bool(torch.isfinite(v).all()), k


@pytest.mark.parametrize("name", hc.CASES)
def test_staged_fp64_agrees_with_head_forward(runs, name):
    """the fp64 restatement and the pinned fp32 `head_forward` are the same head: pooled output to 5e-6 (measured <= 1.4e-6)"""
    hw, rt, dt, s64, s32 = runs[name]
    exp = do.head_forward(hw, rt, dt)
    gap = np.abs(s64["out"].numpy() - exp).max()
    print(f"{name}: |fp64 staged - head_forward| = {gap:.2e}; fp32 staged {np.abs(s32['out'].numpy() - exp).max():.2e}")
    assert gap <= 5e-6


@pytest.mark.parametrize("name", hc.CASES)
def test_swapped_gates_move_the_output(runs, name):
    """a head with rgb_f and depth_f exchanged lands far from the right one on every case (measured 0.32 - 2.75)"""
    hw, rt, dt, s64, _ = runs[name]
    wrong = do.head_stages(hw, rt, dt, torch.float64, swap_gates=True)["out"]
    gap = float((wrong - s64["out"]).abs().max())
    print(f"{name}: swapped gates move the pooled output by {gap:.3f}")
    assert gap > 0.3


def test_borders_saturates_selectors_exactly(runs):
    """fp32 selectors that are exactly 0.0 and exactly 1.0 (x1 == 8 / y1 == 16 with weight 0; expf overflow), 10 of the 48 each"""
    s32, s64 = runs["borders"][4], runs["borders"][3]
    for op in hc.ATTN_OPS:
        sel = s32[op + ".sel"].numpy()
        assert (sel == 0.0).sum() == 10 * B * 128 and (sel == 1.0).sum() == 10 * B * 128, op
        # the other targets land where they were aimed: sel.w ~ N(0, 0.002) moves a logit by 0.002 |q| ~ 0.02 per sigma, the sigmoid's
        # slope is at most 1/4, so 0.05 is ten sigma
        t = hc.border_targets()
        aim = np.concatenate([t[:, 0], t[:, 1]])
        assert np.abs(s64[op + ".sel"].numpy() - aim[None, :]).max() < 0.05


def test_gates_span_the_unit_interval(runs):
    g = runs["gates"][3]["rgb_f"]
    assert float(g.min()) < 0.01 and float(g.max()) > 0.99


def test_offset_drives_the_hyper_network_past_100(runs):
    s = runs["offset"][3]
    assert float(s["h1"].abs().max()) > 100
    assert float(s["cat"][:, 128:].mean()) > 90 and float(s["cat"][:, :128].mean()) < -50


def test_sharp_has_dominant_sampling_points(runs):
    s = runs["sharp"][3]
    assert max(float(s[op + ".aw"].max()) for op in hc.ATTN_OPS) > 0.99
    assert max(float(s[op + ".aw_logits"].abs().max()) for op in hc.ATTN_OPS) > 20


def test_stage_functions_reproduce_head_stages_from_its_own_intermediates(runs):
    """what the GPU test does with the device's taps, done here with the oracle's own: each stage recomputed from its inputs is the
    intermediate itself (bit for bit -- same functions, same inputs)"""
    hw, rt, dt, s, _ = runs["random"]
    h = do.head_weights_as(hw, torch.float64)
    assert torch.equal(do.stage_merge(h, "depth", s["gl"], s["lp"]), s["cat"][:, :128])
    x = s["cat"]
    for i in range(4):
        x = do.stage_hyper(h, i, x)
        assert torch.equal(x, s[f"h{i + 1}"])
    assert torch.equal(do.stage_gates(s["h4"])[0], s["rgb_f"])
    assert torch.equal(do.stage_sample(s["r2d.sel"], s["r2d.aw_logits"], s["v_d"]), s["r2d.samp"])
    fin = do.stage_final(h, s["cat"], s["q_r"], s["v_r"], s["q_d"], s["v_d"], s["rgb_f"], s["depth_f"])
    assert torch.equal(fin["fr"], s["fr"]) and torch.equal(fin["fd"], s["fd"])
    assert torch.equal(do.stage_pool(s["fr"], s["fd"], s["rgb_f"], s["depth_f"]), s["out"])


def test_case_weights_share_the_products_generator():
    from ibloc_amd import dator as D
    a, b = hc.base_weights(), D.random_head_weights(hc.SEED)
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]), k


def test_workspace_layout_is_ordered_aligned_and_inside_the_workspace():
    """ibl_dator_head_workspace_layout (no device call): 19 buffers in the header's order, each on a 256-byte boundary, none overlapping
    the next, the last one ending inside ibl_dator_head_workspace_bytes even when the caller's pointer needs 255 bytes of alignment"""
    from ibloc_amd import _lib
    from ibloc_amd import dator as D
    assert len(D.HEAD_TAPS) == 19
    for batch in (1, 2, 3, 65, 512):
        offs = (ctypes.c_int64 * 19)()
        assert _lib.lib.ibl_dator_head_workspace_layout(batch, offs, 19) == 0
        offs = list(offs)
        R = batch * 128
        sizes = [4 * (w * R if w else R) for _, w in D.HEAD_TAPS]
        sizes[2] = 4 * batch * 128                                   # gl: one row per crop
        assert offs[0] == 0
        for i in range(19):
            assert offs[i] % 256 == 0
            if i:
                assert offs[i - 1] + sizes[i - 1] <= offs[i] < offs[i - 1] + sizes[i - 1] + 256
        assert offs[-1] + sizes[-1] + 255 <= _lib.lib.ibl_dator_head_workspace_bytes(batch)
    two = (ctypes.c_int64 * 2)()
    assert _lib.lib.ibl_dator_head_workspace_layout(4, two, 2) == 0 and two[1] == 4 * 128 * 128 * 4
    assert _lib.lib.ibl_dator_head_workspace_layout(0, two, 2) < 0
    assert _lib.lib.ibl_dator_head_workspace_layout(4, two, 20) < 0
    assert _lib.lib.ibl_dator_head_workspace_layout(4, None, 2) < 0


@pytest.mark.parametrize("shape", hc.DEPTH_SHAPES)
def test_fp32_coordinate_rule_is_the_float64_rule(shape):
    """the depth resize's fp32 source coordinate (oracle.dator_oracle.resize_coords, the kernel's documented rule) against
    (o + 0.5) * n / out - 0.5 in float64: within 4 ulp, and the same first tap wherever the float64 coordinate is further than that from
    an integer -- the convention the GPU value check takes as given"""
    for out, n in ((256, shape[0]), (128, shape[1])):
        i0, i1, fr = do.resize_coords(out, n)
        f64 = (np.arange(out, dtype=np.float64) + 0.5) * n / out - 0.5
        ulp4 = 4 * np.spacing(np.maximum(np.abs(f64), 2.0 ** -126).astype(np.float32)).astype(np.float64)
        inside = (f64 >= 0) & (f64 < n - 1)
        f32 = i0.astype(np.float64) + fr.astype(np.float64)
        assert np.all(np.abs(f32 - f64)[inside] <= ulp4[inside])
        clear = inside & (np.abs(f64 - np.round(f64)) > ulp4)
        assert np.array_equal(i0[clear], np.floor(f64[clear]).astype(np.int64))
        assert np.array_equal(i1[clear], i0[clear] + 1)
        # outside: edge clamp, no interpolation
        lo, hi = f64 < -ulp4, f64 > n - 1 + ulp4
        assert np.all(i0[lo] == 0) and np.all(fr[lo] == 0) and np.all(i0[hi] == n - 1) and np.all(i1[hi] == n - 1) and np.all(fr[hi] == 0)
        assert i0.min() >= 0 and i1.max() <= n - 1 and fr.min() >= 0 and fr.max() < 1


def test_depth_oracles_agree_and_the_numpy_im2col_is_the_patch_layout():
    """the fp64 value reference of the GPU depth test is the fp32 oracle up to fp32 rounding (2e-6, inside the 2^-18 of the GPU test's
    bound), and the independent im2col puts pixel (y, x) of channel c at row (y // 16) * 8 + x // 16, column c * 256 + (y % 16) * 16 + x % 16"""
    d = hc.depth_crop((90, 60), "uniform")
    a, b = do.preprocess_depth(d)[0], do.preprocess_depth_f64(d)
    assert np.abs(a - b).max() < 2e-6
    assert a.min() == -1.0 and a.max() == 1.0                      # both clip ends are hit
    img = np.arange(256 * 128, dtype=np.float32).reshape(256, 128)
    p = hc.im2col(img, 16, 800)
    assert p.shape == (128, 800) and not p[:, 768:].any()
    for y, x, c in [(0, 0, 0), (255, 127, 2), (17, 5, 1), (16, 16, 0), (100, 77, 2)]:
        assert p[(y // 16) * 8 + x // 16, c * 256 + (y % 16) * 16 + x % 16] == img[y, x]
