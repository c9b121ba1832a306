"""-m gpu: the encoder forward and each of its kernels alone give, byte for byte, what they gave before csrc/vit.hip was split into
vit_gemm.hip, vit_layernorm.hip, vit_attention.hip and the staged forward of vit.hip.  Cases: tests/vit_parent_cases.py; the digests of
the earlier commit: tests/golden/vit_parent_digests.json (tools/gen_golden_vit_parent.py, run twice there with identical files).  The
split changed no device instruction and no launch, so there is no tolerance: a digest that differs is a defect."""
import functools
import json

import pytest

from tests import vit_parent_cases as PC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def golden():
    with open(PC.GOLDEN) as f:
        return json.load(f)


def hold(group):
    want = {k: v for k, v in golden().items() if k.startswith(group + "/")}
    got = PC.run_group(group)
    assert sorted(got) == sorted(want), "the cases of the group are not the cases of the golden file"
    bad = sorted(k for k in got if got[k] != want[k])
    assert not bad, f"{len(bad)} of {len(got)} outputs differ from the earlier commit's bytes: {bad}"


def test_golden_is_the_case_table():
    groups = {k.rsplit("/", 1)[0] for k in golden()}
    assert groups == set(PC.GROUPS)


@pytest.mark.parametrize("cfg", PC.STREAM, ids=PC.stream_id)
def test_forward_stream_configs(cfg):
    """every family, plan, launch-per-term and folded-LayerScale form of test_gpu_vit_stream.py: n_blocks_run 0 .. 3, all tokens and class
    rows, with and without the final LayerNorm, clip with its projection"""
    hold("stream/" + PC.stream_id(cfg))


@pytest.mark.parametrize("name", list(PC.FORWARD))
def test_forward_configs(name):
    """V.CONFIGS under `plain` and the default plan: attention tiers 4, 13 and 17, rotation ahead of both attention kernels, registers, no
    class token, and (tiny_dino at batch 17) the 256 x 256 tile inside a forward"""
    hold("forward/" + name)


@pytest.mark.parametrize("shape", list(PC.GEMM_SHAPES))
def test_gemm(shape):
    hold("gemm/" + shape)


@pytest.mark.parametrize("group", ["attention", "attention_stream", "layernorm", "rope"])
def test_kernel(group):
    hold(group)
