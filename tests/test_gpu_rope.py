"""-m gpu: `ibl_rope_f16` (ibl_rope_kernel, csrc/vit_attention.hip) on its own -- every element inside the bound of tests/dino_reg_cases.py against the
fp64 rotation of the same fp16 inputs and fp32 table, everything the kernel must leave alone bit for bit (prefix rows, v columns, a
NaN-filled guard after the last row, q under k_only), the same bytes from two calls and for a crop alone or inside a batch, and every
refusal without a launch."""
import numpy as np
import pytest
import torch

from tests import dino_reg_cases as DC

pytestmark = pytest.mark.gpu
GUARD_ROWS = 3
SENT16 = 0x7E2A                      # an fp16 NaN pattern no kernel writes
GRIDS = {1: (1, 1), 49: (7, 7), 196: (14, 14), 576: (24, 24)}


def _bits(t):
    return t.view(torch.int16)


def _device_buffer(x):
    """x fp16 (B, T, 3D) numpy -> (flat device buffer with GUARD_ROWS NaN rows behind it, its (B, T, 3D) view)"""
    B, T, D3 = x.shape
    flat = torch.full(((B * T + GUARD_ROWS) * D3,), SENT16, dtype=torch.int16, device="cuda").view(torch.float16)
    view = flat[:B * T * D3].view(B, T, D3)
    view.copy_(torch.from_numpy(x))
    return flat, view


def _guard_intact(flat, n):
    return bool((_bits(flat[n:]) == SENT16).all())


@pytest.mark.parametrize("patches", (1, 49, 196, 576))
@pytest.mark.parametrize("prefix", (0, 1, 5))
@pytest.mark.parametrize("batch", (1, 3))
@pytest.mark.parametrize("heads", (2, 16))
def test_rotation_within_bound_and_untouched_regions(heads, batch, prefix, patches):
    from ibloc_amd import vit as V
    T, D = prefix + patches, 64 * heads
    table = V.rope_table(*GRIDS[patches], 100.0)
    d_table = torch.from_numpy(table).cuda()
    worst = 0.0
    for fam in DC.FAMILIES:
        x = DC.rope_inputs(fam, batch, T, heads, seed=1000 * heads + 10 * patches + prefix)
        ref, bound = DC.rope64(x, table, prefix, heads)
        flat, view = _device_buffer(x)
        V.rope_f16(view, d_table, heads, prefix)
        torch.cuda.synchronize()
        got = view.cpu().numpy()
        assert _guard_intact(flat, x.size), "the guard rows after the buffer were written"
        # prefix rows and the v columns: bit for bit (bound 0 there says the same once more for the values)
        assert np.array_equal(got[:, :prefix].view(np.int16), x[:, :prefix].view(np.int16))
        assert np.array_equal(got[..., 2 * D:].view(np.int16), x[..., 2 * D:].view(np.int16))
        err = np.abs(got.astype(np.float64) - ref)
        assert np.isfinite(got).all() and (err <= bound).all(), (fam, float((err - bound).max()))
        live = bound > 0
        worst = max(worst, float((err[live] / bound[live]).max()))
        if fam == "saturate" and patches > 1:           # (the one patch of a 1 x 1 grid sits at the centre: angle 0)
            assert (np.abs(got) == DC.F16_MAX).any(), "the family is meant to reach the clamp"
        # k_only: q as it was, k the bits of the full run
        flat_k, view_k = _device_buffer(x)
        V.rope_f16(view_k, d_table, heads, prefix, k_only=True)
        got_k = view_k.cpu().numpy()
        assert _guard_intact(flat_k, x.size)
        assert np.array_equal(got_k[..., :D].view(np.int16), x[..., :D].view(np.int16))
        assert np.array_equal(got_k[..., D:].view(np.int16), got[..., D:].view(np.int16))
        if fam == "normal":
            # two calls on the same input give the same bytes; a crop alone is the crop inside the batch
            _, again = _device_buffer(x)
            V.rope_f16(again, d_table, heads, prefix)
            assert torch.equal(_bits(again), _bits(view))
            if batch > 1:
                _, alone = _device_buffer(x[1:2])
                V.rope_f16(alone, d_table, heads, prefix)
                assert torch.equal(_bits(alone[0]), _bits(view[1]))
    print(f"heads {heads} batch {batch} prefix {prefix} patches {patches}: worst |got - ref| / bound = {worst:.3f}")


def test_every_refusal_launches_nothing():
    from ibloc_amd import _lib
    from ibloc_amd import vit as V
    heads, prefix, patches = 2, 1, 49
    x = DC.rope_inputs("normal", 2, prefix + patches, heads, seed=5)
    flat, view = _device_buffer(x)
    table = torch.from_numpy(V.rope_table(7, 7, 100.0)).cuda()
    before = _bits(flat).clone()
    q, t, s = view.data_ptr(), table.data_ptr(), torch.cuda.current_stream().cuda_stream
    B, T, D = 2, prefix + patches, 64 * heads
    bad = [(q, t, B, T, prefix, D + 64, heads, 0), (q, t, B, T, prefix, D, heads + 1, 0), (q, t, B, T, prefix, 96, heads, 0),
           (q, t, B, T, prefix, D, 0, 0), (q, t, B, T, -1, D, heads, 0), (q, t, B, T, T + 1, D, heads, 0), (q, t, -1, T, prefix, D, heads, 0),
           (q, t, B, -T, prefix, D, heads, 0), (None, t, B, T, prefix, D, heads, 0), (q, None, B, T, prefix, D, heads, 0),
           (q + 2, t, B, T, prefix, D, heads, 0), (q + 8, t, B, T, prefix, D, heads, 0), (q, t + 4, B, T, prefix, D, heads, 0),
           (q, t, B, T, prefix, D, heads, 2), (q, t, B, T, prefix, D, heads, -1)]
    for args in bad:
        assert _lib.lib.ibl_rope_f16(*args, s) < 0 and _lib.lib.ibl_last_error(), args
    # empty work: no patch rows, no crops
    assert _lib.lib.ibl_rope_f16(q, t, B, T, T, D, heads, 0, s) == 0 and _lib.lib.ibl_rope_f16(q, t, 0, T, prefix, D, heads, 0, s) == 0
    with pytest.raises(_lib.IblError):
        V.rope_f16(view, table, heads + 1, prefix)
    torch.cuda.synchronize()
    assert torch.equal(_bits(flat), before)
