"""`ibl_preprocess_crops_ragged` (native-aspect crops: every crop resized whole to its own multiple of the patch size, its patches
written at its own rows of a per-token patch matrix): the u8 image of every crop equals PIL.Image.resize bit for bit, the patch rows
equal the im2col of the normalised image rounded to fp16, the prefix rows and the K padding are zero, and an equal-size batch under
an "exact" recipe equals `ibl_preprocess_crops`."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu

# (source h x w, grid): sources smaller and larger than the target, single-row, single-column and single-patch grids
CASES = [((5, 5), (1, 1)), ((40, 60), (1, 9)), ((480, 160), (9, 1)), ((700, 300), (16, 16)), ((480, 160), (27, 9)), ((40, 60), (16, 16)),
         ((5, 5), (27, 9)), ((700, 300), (1, 1)), ((14, 126), (1, 9))]     # the last one: both passes are the identity


def _encoder(cfg_name, recipe):
    from ibloc_amd import vit as V
    cfg = dataclasses.replace(V.CONFIGS[cfg_name], recipe=recipe)
    return V.VitEncoder(cfg, V.random_weights(cfg, 1))


@pytest.mark.parametrize("cfg_name,recipe", [("tiny_dino", "dinov2"), ("tiny_dino_reg", "dinov2"), ("tiny_dino", "vit")])
def test_u8_and_patch_rows_vs_pil(cfg_name, recipe):
    """dinov2: bicubic, ImageNet mean / std; vit: bilinear, mean = std = 0.5; tiny_dino_reg: five prefix rows per crop"""
    enc = _encoder(cfg_name, recipe)
    cfg, r, p = enc.cfg, enc.recipe, enc.cfg.patch
    rng = np.random.default_rng(21)
    crops = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for (h, w), _ in CASES]
    grids = [g for _, g in CASES]
    patches, imgs = enc.preprocess_ragged(crops, grids, want_u8=True)
    torch.cuda.synchronize()
    seq = enc.seq_offsets(grids)
    got = patches.cpu().numpy()
    assert got.shape == (int(seq[-1]), cfg.patch_k_pad)
    written = np.zeros(got.shape[0], bool)
    for i, (c, (gh, gw)) in enumerate(zip(crops, grids)):
        exact = dataclasses.replace(r, resize_mode="exact", out_h=gh * p, out_w=gw * p)
        want_u8 = vo.preprocess_crop_u8(c, exact)             # the swap, then ONE PIL resize of the whole crop
        assert np.array_equal(imgs[i].cpu().numpy(), want_u8), f"crop {i} {c.shape[:2]} -> grid {(gh, gw)}: u8 image"
        x = vo.preprocess_crop(c, exact)                      # (3, gh p, gw p) fp32, normalised
        want = x.reshape(3, gh, p, gw, p).transpose(1, 3, 0, 2, 4).reshape(gh * gw, 3 * p * p).astype(np.float16)
        lo = int(seq[i]) + cfg.n_prefix
        assert np.array_equal(got[lo:lo + gh * gw, :cfg.patch_k].view(np.uint16), want.view(np.uint16)), f"crop {i}: patch rows"
        assert lo + gh * gw == int(seq[i + 1])
        written[lo:lo + gh * gw] = True
    assert (got[~written].view(np.uint16) == 0).all(), "prefix rows are not zero"
    assert (~written).sum() == len(CASES) * cfg.n_prefix
    assert (got[:, cfg.patch_k:].view(np.uint16) == 0).all(), "K padding is not zero"


def test_equal_sizes_under_an_exact_recipe_are_the_fixed_entry():
    enc = _encoder("tiny_dino", "vit")
    cfg = enc.cfg
    rng = np.random.default_rng(22)
    crops = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in [(224, 224), (64, 400), (333, 97), (5, 5), (500, 375)]]
    fixed = enc.preprocess(crops).cpu().numpy().view(np.uint16).reshape(len(crops), cfg.n_patches, -1)
    ragged = enc.preprocess_ragged(crops, [cfg.grid] * len(crops)).cpu().numpy().view(np.uint16).reshape(len(crops), cfg.n_tokens, -1)
    assert np.array_equal(ragged[:, cfg.n_prefix:], fixed)
    assert (ragged[:, :cfg.n_prefix] == 0).all()


def test_refusals_launch_nothing():
    from ibloc_amd import _lib
    from ibloc_amd import preprocess as pp
    enc = _encoder("tiny_dino", "dinov2")
    cfg, r = enc.cfg, enc.recipe
    shapes, sizes = [(30, 40), (50, 20)], [(28, 42), (42, 14)]
    rows = 1 + 6 + 1 + 3
    src = torch.zeros(sum(h * w * 3 for h, w in shapes), dtype=torch.uint8, device="cuda")
    patches = torch.full((rows, cfg.patch_k_pad), 7.0, dtype=torch.float16, device="cuda")
    mean, std = (C.c_float * 3)(*r.mean), (C.c_float * 3)(*r.std)
    st = torch.cuda.current_stream().cuda_stream

    def call(sizes=sizes, row0s=(1, 8), patch_rows=rows, null=None):
        descs, rdescs, tables, _, tmp_bytes, _, max_h = pp.plan_batch_ragged(r, shapes, sizes, row0s)
        dev = lambda s: torch.frombuffer(bytearray(bytes(s)), dtype=torch.uint8).cuda()
        d_descs, d_rdescs, d_tables = dev(descs), dev(rdescs), torch.from_numpy(tables).cuda()
        tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device="cuda")
        args = dict(src=src.data_ptr(), descs=d_descs.data_ptr(), rdev=d_rdescs.data_ptr(), rhost=C.addressof(rdescs), tables=d_tables.data_ptr(),
                    tmp=tmp.data_ptr(), patches=patches.data_ptr())
        if null:
            args[null] = None
        return _lib.lib.ibl_preprocess_crops_ragged(args["src"], args["descs"], args["rdev"], args["rhost"], len(shapes), max_h, args["tables"],
                                                    args["tmp"], cfg.patch, cfg.patch_k_pad, 1, mean, std, args["patches"], patch_rows, None, st)

    for null in ("src", "descs", "rdev", "rhost", "tables", "tmp", "patches"):
        assert call(null=null) < 0 and b"null" in _lib.lib.ibl_last_error(), null
    assert call(sizes=[(28, 42), (40, 14)]) < 0                  # 40 is no multiple of the patch size
    assert call(row0s=(1, 6)) < 0 and b"ascending" in _lib.lib.ibl_last_error()     # crop 0 takes rows 1 .. 6
    assert call(row0s=(8, 1)) < 0
    assert call(patch_rows=rows - 1) < 0                         # the last crop would end beyond the matrix
    torch.cuda.synchronize()
    assert (patches.cpu().numpy() == 7.0).all(), "a refused call wrote to the patch matrix"
    assert call() == 0
    torch.cuda.synchronize()
    assert (patches[0].cpu().numpy() == 0).all() and (patches[7].cpu().numpy() == 0).all()
