"""-m gpu: a descriptor that `ibl_vit_forward` refuses for the operand terms of ONE layer is refused before anything is launched: the
status and the message name the layer, and neither the workspace nor `out` has a byte written.  (The terms of every block to run are
decided and validated ahead of the patch embedding; checked inside the block loop, layer l was refused only after the patch embedding and
blocks 0 .. l - 1 had written into the caller's workspace.)"""
import ctypes as C

import pytest
import torch

from ibloc_amd import _lib
from ibloc_amd import vit as V
from tests import vit_stream_cases as SCS

pytestmark = pytest.mark.gpu
IBL_ERR_ARG = -1
PATTERN = 0xA5


def refused(mutate):
    """the stream family `vit` (17 tokens, batch 3), plan p2;1:1313, all tokens, `mutate(enc)` applied after construction -> (status,
    message, workspace bytes, out bytes) of a direct call"""
    m = SCS.Model("vit", "p2;1:1313")
    enc = V.VitEncoder(SCS.run_cfg("vit", SCS.DEPTH, True), m.w, precision="p2;1:1313")
    mutate(enc)
    patches = torch.from_numpy(m.patches).cuda()
    ws = torch.full((_lib.lib.ibl_vit_workspace_bytes(C.byref(enc.desc), SCS.BATCH),), PATTERN, dtype=torch.uint8, device="cuda")
    out = torch.full((SCS.BATCH * m.T * m.D * 4,), PATTERN, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = _lib.lib.ibl_vit_forward(C.byref(enc.desc), C.byref(enc.W), patches.data_ptr(), SCS.BATCH, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                  torch.cuda.current_stream().cuda_stream)
    msg = _lib.lib.ibl_last_error().decode()
    torch.cuda.synchronize()
    return st, msg, ws.cpu(), out.cpu()


def untouched(ws, out):
    return bool((ws == PATTERN).all()) and bool((out == PATTERN).all())


def test_act_terms_flag_missing():
    """layer 1 runs o and fc2 in three terms; without IBL_VIT_ACT_TERMS3 the workspace has no room for their rows"""
    def clear(enc):
        assert enc.desc.flags & V.FLAG_ACT_TERMS3
        enc.desc.flags &= ~V.FLAG_ACT_TERMS3

    st, msg, ws, out = refused(clear)
    assert st == IBL_ERR_ARG
    assert msg == "ibl_vit_forward: layer 1: o_terms / fc2_terms 3 / 3 need IBL_VIT_ACT_TERMS3 in the descriptor"
    assert untouched(ws, out), "refused, but the patch embedding and block 0 had already written"


def test_four_operand_terms():
    """qkv_terms = 4 set by hand on layer 2 (with a K-extended weight pointer, or the count is not read)"""
    def four(enc):
        L = enc.W.layers[2]
        L.w_qkv_x, L.qkv_terms = L.w_qkv, 4

    st, msg, ws, out = refused(four)
    assert st == IBL_ERR_ARG
    assert msg == "ibl_vit_forward: layer 2: at most three operand terms"
    assert untouched(ws, out), "refused, but the patch embedding and blocks 0 and 1 had already written"
