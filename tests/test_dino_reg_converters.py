"""CPU: the converters of the register / rotary checkpoints (utils/embeddings.py), what load_encoder refuses before any upload, and the
C-ABI additions (ibl_vit_desc.n_registers, ibl_vit_weights.reg_tokens / rope_table, ibl_rope_f16) against include/ibloc.h."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from ibloc_amd import vit as V
from ibloc_amd.utils import embeddings as E
from tests import dino_reg_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["tiny_dino_reg", "tiny_dinov3"])
def test_converter_output_is_the_restatements_weights(name):
    """through the state dict of the transformers model itself (so the names are the installed version's), bit for bit"""
    cfg = V.CONFIGS[name]
    w = DC.seeded_weights(cfg, 7)
    sd = DC.hf_model(cfg, w).state_dict()
    conv = E.hf_dinov3_to_weights if cfg.rope_theta is not None else E.hf_dinov2_to_weights
    got = conv(sd, cfg.depth)
    assert sorted(got) == sorted(w)
    for k in w:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], w[k]), k
    assert got["reg"].shape == (4, cfg.dim)
    E.check_dino_weights(got, cfg)
    if cfg.rope_theta is not None:
        assert "pos" not in got and not any("k_proj.bias" in k for k in sd)
        for l in range(cfg.depth):
            b_qkv = np.concatenate([got[f"l{l}.{n}.b"] for n in "qkv"])
            assert not b_qkv[cfg.dim:2 * cfg.dim].any() and b_qkv[:cfg.dim].any() and b_qkv[2 * cfg.dim:].any()
    # the hub layout's name for the registers
    if cfg.rope_theta is None:
        sd2 = dict(sd)
        sd2["register_tokens"] = sd2.pop("embeddings.register_tokens")
        assert np.array_equal(conv(sd2, cfg.depth)["reg"], w["reg"])


def test_plain_dinov2_state_dict_converts_as_before():
    cfg = V.CONFIGS["tiny_dino"]
    w = V.random_weights(cfg, 7)
    sd = {k: v for k, v in DC.hf_dinov2_reg_state_dict(cfg, dict(w, reg=np.zeros((0, cfg.dim), np.float32))).items() if "register" not in k}
    got = E.hf_dinov2_to_weights(sd, cfg.depth)
    assert "reg" not in got and sorted(got) == sorted(w) and all(np.array_equal(got[k], w[k]) for k in w)


def test_refusals_before_any_upload():
    """each raises ValueError naming the reason; load_encoder reaches no device (this test runs without one)"""
    import dataclasses
    reg, v3 = V.CONFIGS["tiny_dino_reg"], V.CONFIGS["tiny_dinov3"]
    sd_reg = DC.hf_state_dict(reg, DC.seeded_weights(reg, 1))
    sd_v3 = DC.hf_state_dict(v3, DC.seeded_weights(v3, 1))
    old = dict(E._ENCODERS)
    # gated MLP: DINOv3 S+ / H+ (gate_proj), DINOv2-g (SwiGLU weights_in)
    with pytest.raises(ValueError, match="gated MLP"):
        E.load_encoder("dinov3", dict(sd_v3, **{"model.layer.0.mlp.gate_proj.weight": torch.zeros(256, 128)}), device="cpu", cfg="tiny_dinov3")
    with pytest.raises(ValueError, match="gated MLP"):
        E.load_encoder("dino", dict(sd_reg, **{"encoder.layer.0.mlp.weights_in.weight": torch.zeros(512, 128)}), device="cpu", cfg="tiny_dino_reg")
    # head_dim != 64
    with pytest.raises(ValueError, match="head_dim"):
        E.load_encoder("dinov3", sd_v3, device="cpu", cfg=dataclasses.replace(v3, heads=4))
    with pytest.raises(ValueError, match="head_dim"):
        E.load_encoder("dino", sd_reg, device="cpu", cfg=dataclasses.replace(reg, heads=1))
    # register count: a register checkpoint under a plain configuration, a plain one under a register configuration, 4 against 2
    with pytest.raises(ValueError, match="register tokens"):
        E.load_encoder("dino", sd_reg, device="cpu", cfg="tiny_dino")
    plain = {k: v for k, v in sd_reg.items() if "register" not in k}
    with pytest.raises(ValueError, match="register tokens"):
        E.load_encoder("dino", plain, device="cpu", cfg="tiny_dino_reg")
    with pytest.raises(ValueError, match="register tokens"):
        E.load_encoder("dinov3", sd_v3, device="cpu", cfg=dataclasses.replace(v3, n_registers=2))
    assert E._ENCODERS == old


def test_new_fields_match_the_header(tmp_path):
    """sizes of the two structs and the offsets of the appended fields, from a C program compiled against include/ibloc.h"""
    src = tmp_path / "fields.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ibloc.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ibl_vit_desc), offsetof(ibl_vit_desc, ln_eps), offsetof(ibl_vit_desc, n_registers),\n'
                   '         sizeof(ibl_vit_weights), offsetof(ibl_vit_weights, layers), offsetof(ibl_vit_weights, reg_tokens), offsetof(ibl_vit_weights, rope_table));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "fields"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D, W = V.VitDesc, V.VitWeights
    assert got == [ctypes.sizeof(D), D.ln_eps.offset, D.n_registers.offset, ctypes.sizeof(W), W.layers.offset, W.reg_tokens.offset, W.rope_table.offset]
    # appended: the fields before them sit where they sat, and the last fields of the mirrors are the new ones
    assert D._fields_[-1][0] == "n_registers" and (D.ln_eps.offset, D.n_registers.offset) == (48, 52)
    assert [f[0] for f in W._fields_[-2:]] == ["reg_tokens", "rope_table"] and W.reg_tokens.offset == W.layers.offset + ctypes.sizeof(V.VitLayer) * V.MAX_LAYERS
    # positional construction of before the field existed leaves it 0
    assert V.VitDesc(128, 2, 2, 256, 14, 224, 224, 257, 640, 0, 2, 128, 1e-6).n_registers == 0


def test_rope_entry_refuses_without_a_gpu():
    """ibl_rope_f16 is exported and decides every refusal before any HIP call; empty work is IBL_OK"""
    from ibloc_amd import _lib
    lib = _lib.lib
    buf = np.zeros(4096, dtype=np.uint8)
    p = (buf.ctypes.data + 15) & ~15                          # host memory, never dereferenced: every call is refused or empty
    for args in [(p, p, 1, 10, 1, 128, 3, 0), (p, p, 1, 10, 1, 100, 2, 0), (p, p, 1, 10, 11, 128, 2, 0), (p, p, 1, 10, -1, 128, 2, 0),
                 (p, p, -1, 10, 1, 128, 2, 0), (p, p, 1, -10, 1, 128, 2, 0), (None, p, 1, 10, 1, 128, 2, 0), (p, None, 1, 10, 1, 128, 2, 0),
                 (p + 2, p, 1, 10, 1, 128, 2, 0), (p, p + 4, 1, 10, 1, 128, 2, 0), (p, p, 1, 10, 1, 128, 2, 2), (p, p, 1, 10, 1, 128, 0, 0)]:
        assert lib.ibl_rope_f16(*args, None) < 0 and lib.ibl_last_error(), args
    assert lib.ibl_rope_f16(p, p, 0, 10, 1, 128, 2, 0, None) == 0 and lib.ibl_rope_f16(None, None, 3, 10, 10, 128, 2, 0, None) == 0
    assert not buf.any()
