"""`ibl_attention_ragged_f16` (the streaming attention over crops of different lengths packed back to back, on its own): every crop
equals `ibl_attention_stream_f16` run on that crop alone bit for bit -- so no crop reads a neighbour's keys -- and every element of a
mixed batch is within the bound of tests/attention_cases.py of a float64 softmax(q k^T / 8) v, with no allowed share of misses.
A segment table of batch + 1 ascending offsets leaves no rows between two segments: the rows no kernel may touch are those before
seq_off[0] and after seq_off[batch], and both hold the sentinel afterwards.  Every case prints its worst error / bound (run with -s)."""
import numpy as np
import pytest
import torch

from tests import attention_long_cases as LC

pytestmark = pytest.mark.gpu

SENTINEL = 0x7E2A            # an fp16 NaN pattern no kernel writes (the scheme of tests/test_gpu_attention_long.py)
MIXED = (((1, 17, 64, 65, 127, 128, 129, 257, 273, 577), 2), ((273, 1, 130), 16))
FAMILIES = ("peaked", "ramp", "stair_up")
G = 3                        # guard rows on either side


def _packed(family, lengths, heads):
    """the crops of `lengths`, each the (T, heads, 1) case of the family, back to back -> (total, 3 * D) fp16"""
    parts = []
    for T in lengths:
        c = LC.case(family, T, heads, 1)[0]
        parts.append(LC.pack(c["q"], c["k"], c["v"])[0])
    return np.ascontiguousarray(np.concatenate(parts, axis=0))


def _run(qkv_np, lengths, heads, cls_only=False, terms=1):
    """qkv_np (total, 3 * D) -> (out (total, terms * D), the whole guarded buffer as uint16 rows): G sentinel rows lie in front of
    seq_off[0] and behind seq_off[batch], in qkv (as NaN rows) and in out"""
    from ibloc_amd import vit as V
    total, D = qkv_np.shape[0], qkv_np.shape[1] // 3
    assert total == sum(lengths)
    seq = (G + np.concatenate([[0], np.cumsum(lengths)])).astype(np.int32)
    nan_rows = np.full((G, 3 * D), SENTINEL, np.uint16).view(np.float16)
    qkv = torch.from_numpy(np.concatenate([nan_rows, qkv_np, nan_rows])).cuda()
    buf = torch.full((total + 2 * G, terms * D), SENTINEL, dtype=torch.int16, device="cuda")
    V.attention_ragged_f16(qkv, seq, heads, cls_only=cls_only, terms=terms, out=buf.view(torch.float16))
    torch.cuda.synchronize()
    rows = buf.cpu().numpy().view(np.uint16)
    return rows[G:G + total].view(np.float16), rows


def _alone(qkv_np, lengths, heads, terms=1):
    """every crop through the streaming entry on its own (batch 1) -> (total, terms * D)"""
    from ibloc_amd import vit as V
    outs, lo = [], 0
    for T in lengths:
        one = torch.from_numpy(np.ascontiguousarray(qkv_np[lo:lo + T][None])).cuda()
        outs.append(V.attention_stream_f16(one, heads, terms=terms)[0].cpu().numpy())
        lo += T
    return np.concatenate(outs, axis=0)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint16), np.ascontiguousarray(b).view(np.uint16))


@pytest.mark.parametrize("terms", (1, 2, 3))
@pytest.mark.parametrize("T", (289, 17))
def test_equal_lengths_are_the_streaming_entry(T, terms):
    from ibloc_amd import vit as V
    H, B = 2, 3
    c = LC.case("peaked", T, H, B)[0]
    qkv = LC.pack(c["q"], c["k"], c["v"])
    want = V.attention_stream_f16(torch.from_numpy(qkv).cuda(), H, terms=terms).cpu().numpy()
    got, rows = _run(np.ascontiguousarray(qkv.reshape(B * T, -1)), (T,) * B, H, terms=terms)
    assert _same(got, want.reshape(B * T, -1))
    assert (rows[:G] == SENTINEL).all() and (rows[-G:] == SENTINEL).all(), "guard rows written"


@pytest.mark.parametrize("terms", (1, 3))
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("lengths,H", MIXED)
def test_mixed_lengths_each_crop_is_the_crop_alone(lengths, H, family, terms):
    qkv = _packed(family, lengths, H)
    got, rows = _run(qkv, lengths, H, terms=terms)
    want = _alone(qkv, lengths, H, terms=terms)
    lo = 0
    for T in lengths:
        assert _same(got[lo:lo + T], want[lo:lo + T]), f"crop of {T} rows at {lo} != the crop alone ({family}, terms {terms})"
        lo += T
    assert (rows[:G] == SENTINEL).all() and (rows[-G:] == SENTINEL).all(), "guard rows written"


def test_loud_neighbours_do_not_leak():
    """every second crop holds the `offset` family's rows, whose logits carry a common +60: one leaked key would own the softmax"""
    lengths, H = MIXED[0]
    parts = []
    for i, T in enumerate(lengths):
        c = LC.case("offset" if i % 2 else "peaked", T, H, 1)[0]
        parts.append(LC.pack(c["q"], c["k"], c["v"])[0])
    qkv = np.ascontiguousarray(np.concatenate(parts, axis=0))
    got, _ = _run(qkv, lengths, H)
    assert _same(got, _alone(qkv, lengths, H))
    lo = 0
    for i, T in enumerate(lengths):
        _, ref, _, _, bnd, _ = LC.case("offset" if i % 2 else "peaked", T, H, 1)
        a = LC.unpack_out(got[lo:lo + T][None], H)[0]
        assert (np.abs(a.astype(np.float64) - ref) <= bnd).all(), f"crop {i} ({T} rows) misses its fp64 bound beside a loud neighbour"
        lo += T


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("lengths,H", MIXED)
def test_mixed_batch_vs_fp64(lengths, H, family):
    got, _ = _run(_packed(family, lengths, H), lengths, H)
    assert np.isfinite(got.astype(np.float32)).all()
    worst, lo = 0.0, 0
    for T in lengths:
        _, ref, _, _, bnd, _ = LC.case(family, T, H, 1)
        a = LC.unpack_out(got[lo:lo + T][None], H)[0]
        worst = max(worst, float((np.abs(a.astype(np.float64) - ref) / bnd).max()))
        lo += T
    print(f"ragged attention vs fp64: segments {lengths} heads {H} {family}: worst error / bound {worst:.3f}")
    assert worst <= 1.0, (lengths, family, worst)


@pytest.mark.parametrize("terms", (1, 2, 3))
@pytest.mark.parametrize("lengths,H", MIXED)
def test_cls_only_writes_the_class_rows_alone(lengths, H, terms):
    qkv = _packed("ramp", lengths, H)
    full, _ = _run(qkv, lengths, H, terms=terms)
    got, rows = _run(qkv, lengths, H, cls_only=True, terms=terms)
    first = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    assert _same(got[first], full[first]), "class rows != the full run's"
    keep = np.ones(rows.shape[0], bool)
    keep[G + first] = False
    assert (rows[keep] == SENTINEL).all(), "cls_only wrote outside the class rows"


def test_deterministic():
    lengths, H = MIXED[0]
    qkv = _packed("peaked", lengths, H)
    for terms in (1, 3):
        assert _same(_run(qkv, lengths, H, terms=terms)[0], _run(qkv, lengths, H, terms=terms)[0])


def test_refusals_launch_nothing():
    from ibloc_amd import _lib
    call = _lib.lib.ibl_attention_ragged_f16
    st = torch.cuda.current_stream().cuda_stream
    D, H, total = 128, 2, 600
    qkv = torch.zeros((total, 3 * D), dtype=torch.float16, device="cuda")
    buf = torch.full((total * D + 64,), SENTINEL, dtype=torch.int16, device="cuda")
    q, o = qkv.data_ptr(), buf.data_ptr()

    def refused(seq, q=q, o=o, batch=None, dim=D, heads=H, cls_only=0, terms=1, dev=True, host=True):
        seq = np.asarray(seq, dtype=np.int32)
        d = torch.from_numpy(seq).cuda()
        s = call(q, o, d.data_ptr() if dev else None, seq.ctypes.data if host else None, seq.size - 1 if batch is None else batch, dim, heads,
                 cls_only, terms, st)
        assert s < 0 and _lib.lib.ibl_last_error(), (seq, s)

    ok = [0, 300, 600]
    refused(ok, q=None); refused(ok, o=None); refused(ok, dev=False); refused(ok, host=False)      # null pointers
    assert b"null" in _lib.lib.ibl_last_error()
    refused(ok, q=q + 2); refused(ok, o=o + 4)                                                     # misaligned rows
    refused(ok, heads=3)                                                                           # dim != 64 * heads
    refused(ok, terms=0); refused(ok, terms=4)
    refused(ok, cls_only=2)
    refused(ok, batch=-1)
    refused([0, 300, 300]); refused([0, 300, 200])                                                 # an empty, a descending segment
    refused([-1, 300, 600])
    big = torch.zeros((LC.MAX_TOKENS + 1, 3 * D), dtype=torch.float16, device="cuda")
    bigbuf = torch.full(((LC.MAX_TOKENS + 1) * D,), SENTINEL, dtype=torch.int16, device="cuda")
    refused([0, LC.MAX_TOKENS + 1], q=big.data_ptr(), o=bigbuf.data_ptr())                         # one token beyond the limit
    seq = np.asarray(ok, dtype=np.int32)
    assert call(q, o, torch.from_numpy(seq).cuda().data_ptr(), seq.ctypes.data, 0, D, H, 0, 1, st) == 0      # nothing to do
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint16) == SENTINEL).all() and (bigbuf.cpu().numpy().view(np.uint16) == SENTINEL).all()
