"""CPU: host-side logic of the product (resample tables vs PIL, recipes, sharding helpers, gloo all-gather)."""
import os
import subprocess
import sys

import numpy as np
from PIL import Image

from ibloc_amd import preprocess as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _emulate(img, recipe):
    h, w, _ = img.shape
    rh, rw, top, left = pp.resized_size(recipe, h, w)

    def one_pass(arr, in_size, out_size, win0, win_n, axis):
        if in_size == out_size:
            return np.take(arr, np.arange(win0, win0 + win_n), axis=axis)
        rec, ks = pp.resample_table(in_size, out_size, recipe.filt, win0, win_n)
        arr = np.moveaxis(arr, axis, 0).astype(np.int64)
        out = np.zeros((win_n,) + arr.shape[1:], dtype=np.int64)
        for i in range(win_n):
            x0, n = rec[i, 0], rec[i, 1]
            acc = np.full(arr.shape[1:], 1 << (pp.PRECISION_BITS - 1), dtype=np.int64)
            for t in range(n):
                acc += arr[x0 + t] * int(rec[i, 2 + t])
            out[i] = np.clip(acc >> pp.PRECISION_BITS, 0, 255)
        return np.moveaxis(out.astype(np.uint8), 0, axis)

    return one_pass(one_pass(img, w, rw, left, recipe.out_w, 1), h, rh, top, recipe.out_h, 0)


def test_resample_tables_are_bit_exact_vs_pil():
    rng = np.random.default_rng(0)
    for name in ("dinov2", "vit", "clip", "dator_rgb"):
        r = pp.RECIPES[name]
        for (h, w) in [(224, 224), (64, 400), (333, 97), (500, 375), (257, 300)]:
            img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
            rh, rw, top, left = pp.resized_size(r, h, w)
            res = Image.fromarray(img).resize((rw, rh), resample=Image.BICUBIC if r.filt == "bicubic" else Image.BILINEAR)
            ref = np.asarray(res)[top:top + r.out_h, left:left + r.out_w]
            assert np.array_equal(_emulate(img, r), ref), (name, h, w)


def test_native_and_batched_table_builders_equal_the_pil_checked_one():
    """the three builders of the same table -- the scalar numpy form the PIL test above pins, the batch-vectorised numpy form and the
    library's host function `ibl_resample_table` (csrc/resample.cpp, what plan_batch uses) -- agree entry for entry over every recipe and
    2 000 crop sizes, extreme aspect ratios included"""
    rng = np.random.default_rng(1)
    keys = set()
    for _ in range(500):
        h, w = int(rng.integers(8, 900)), int(rng.integers(8, 900))
        for name in ("dinov2", "clip", "vit", "dator_rgb"):
            r = pp.RECIPES[name]
            try:
                rh, rw, top, left = pp.resized_size(r, h, w)
            except ValueError:
                continue
            keys |= {k for k in ((w, rw, r.filt, left, r.out_w), (h, rh, r.filt, top, r.out_h)) if k[0] != k[1]}
    keys = sorted(keys)
    native, batched = pp.resample_tables_native(keys), pp.resample_tables(keys)
    for k in keys:
        assert native[k][1] == batched[k][1] and np.array_equal(native[k][0], batched[k][0]), k
    for k in keys[::40]:
        rec, ksize = pp.resample_table(*k)
        assert ksize == native[k][1] and np.array_equal(rec, native[k][0]), k


def test_plan_batch_shares_tables():
    descs, tables, src_bytes, tmp_bytes, max_h = pp.plan_batch(pp.RECIPES["dinov2"], [(224, 224)] * 5 + [(100, 300)])
    assert descs[0].h_table == descs[4].h_table and descs[5].h_table != descs[0].h_table
    assert src_bytes == 5 * 224 * 224 * 3 + 100 * 300 * 3 and max_h == 224


def test_shard_ranges_cover_everything():
    from ibloc_amd.parallel import shard_range
    for n in (0, 1, 7, 1000, 50001):
        for w in (1, 2, 8):
            got = [shard_range(n, r, w) for r in range(w)]
            assert got[0][0] == 0 and got[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(got[:-1], got[1:]))
            assert max(b - a for a, b in got) - min(b - a for a, b in got) <= 1


WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["IBL_ROOT"])
import numpy as np, torch, torch.distributed as dist
from ibloc_amd.parallel import shard_range, allgather_similarity_blocks, augment_half, frames_for_rank
from ibloc_amd.assign import assign_batch
from oracle import match_oracle as mo
from oracle import simvolume_oracle as so
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
rng = np.random.default_rng(5)
M, E, D, Q = 37, 3, 64, 5
mem = mo.normalize_rows(rng.normal(size=(M * E, D)).astype(np.float32))
det = mo.normalize_rows(rng.normal(size=(Q, D)).astype(np.float32))
off = (np.arange(M + 1) * E).astype(np.int32)
lo, hi = shard_range(M, rank, world)
local = mo.closest_similarity(det, mem[lo * E:hi * E], (off[lo:hi + 1] - off[lo]).astype(np.int32))   # this rank's instance shard
full = allgather_similarity_blocks(torch.from_numpy(local), M)
exp = mo.closest_similarity(det, mem, off)
assert np.array_equal(full.numpy(), exp), "gathered similarity matrix differs"
aug = augment_half(full)
got = assign_batch(aug[None], [Q], 4, 1)[0]
assert got == so.simvolume_assignments(exp, 4)
assert list(frames_for_rank(10, rank, world)) == list(range(*shard_range(10, rank, world)))
dist.barrier()
if rank == 0:
    print("GLOO_OK")
dist.destroy_process_group()
'''


def test_sharded_match_allgather_gloo_world2(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, IBL_ROOT=ROOT, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                          "127.0.0.1", "--master-port", "29517", str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "GLOO_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


EVAL_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["IBL_ROOT"])
import numpy as np, torch, torch.distributed as dist
from ibloc_amd.parallel import evaluate_sharded, fitness_rmse_from_d2, shard_range
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
rng = np.random.default_rng(9)                       # same data on every rank
M, sizes, thr = 11, [400, 250, 0, 333], 0.05
mem = [rng.uniform(-1, 1, size=(300, 3)) for _ in range(M)]
det = rng.uniform(-1, 1, size=(sum(sizes), 3))
def d2_against(points):                              # what ibl_evaluate_batch writes to d2_out for a shard: nearest squared distance within thr
    d = ((det[:, None, :].astype(np.float32) - points[None, :, :].astype(np.float32)) ** 2).sum(-1).min(axis=1)
    d[d >= np.float32(thr * thr)] = np.inf
    return torch.from_numpy(d.astype(np.float32))
lo, hi = shard_range(M, rank, world)
local = d2_against(np.concatenate(mem[lo:hi])) if hi > lo else torch.full((len(det),), float("inf"))
fit, rmse = evaluate_sharded(local, sizes)
want_fit, want_rmse = fitness_rmse_from_d2(d2_against(np.concatenate(mem)), sizes)
assert np.array_equal(fit, want_fit) and np.allclose(rmse, want_rmse, rtol=1e-12, atol=0), (fit, want_fit)
assert fit[2] == 0.0 and rmse[2] == 0.0 and 0 < fit[0] < 1
dist.barrier()
if rank == 0:
    print("EVAL_OK")
dist.destroy_process_group()
'''


def test_sharded_evaluate_allreduce_min_gloo_world2(tmp_path):
    """memory clouds sharded by instance range, per-point nearest distances combined with all-reduce(MIN)"""
    script = tmp_path / "eval_worker.py"
    script.write_text(EVAL_WORKER)
    env = dict(os.environ, IBL_ROOT=ROOT, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                          "127.0.0.1", "--master-port", "29519", str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "EVAL_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


TOPK_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["IBL_ROOT"])
import numpy as np, torch, torch.distributed as dist
from ibloc_amd.assign import assign_batch, assign_candidates
from ibloc_amd.parallel import ShardExchange, shard_range, sharded_candidates
from tests.test_assign_candidates import select_np
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
K_HI, K_LO, CAP = 192, 32, 24
QUANT = 0
rng = np.random.default_rng(77)                      # same memory on every rank
M, E, D = 1501, 2, 48
base = rng.normal(size=(M, D))
mem = base[:, None, :] + rng.normal(0, 0.3, size=(M, E, D))
mem /= np.linalg.norm(mem, axis=-1, keepdims=True)
lo, hi = shard_range(M, rank, world)

def full_rows(q):                                    # [closest similarity | 1] in fp16 against a range of instances
    def rows(a, b):
        s = np.einsum("qd,med->qme", q.astype(np.float32), mem[a:b].astype(np.float32)).max(-1)
        if QUANT:
            s = np.where(s > 0.6, 0.75, 0.5)             # two similarity levels only: every row ties massively at the threshold
        out = np.ones((len(q), b - a + 1), dtype=np.float16)
        out[:, :-1] = s
        return out
    return rows

def match_local(allq):                               # what ibl_match_topk does on the GPU, restated with numpy
    aug = full_rows(allq.numpy())(lo, hi)
    R, S = len(aug), K_HI + K_LO
    val, idx, cnt = np.zeros((R, S), np.float16), np.full((R, S), -1, np.int32), np.zeros((R, 2), np.int32)
    for r in range(R):
        v, j = select_np(aug[r, :-1], lo, K_HI, K_LO)
        val[r, :len(v)], idx[r, :len(v)] = v, j
        cnt[r] = (K_HI, K_LO) if hi - lo > S else (hi - lo, 0)
    return torch.from_numpy(val), torch.from_numpy(idx), torch.from_numpy(cnt), torch.from_numpy(aug)

ex = ShardExchange(None, CAP)
frng = np.random.default_rng(100 + rank)             # every rank has its own frames
for step, kind in enumerate(["reid", "ties"]):
    q_per_frame = np.array([7, 3, 1, 5] if rank == 0 else [2, 7, 7], dtype=np.int32)
    ids = frng.integers(0, M, size=int(q_per_frame.sum()))
    q = base[ids] + frng.normal(0, 0.25, size=(len(ids), D))
    QUANT = 2 if kind == "ties" else 0
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    detn = torch.from_numpy(q.astype(np.float32))
    val_h, idx_h, cnt_h, aug_local = sharded_candidates(ex, detn, match_local)
    row0 = np.concatenate([[0], np.cumsum(q_per_frame)]).astype(np.int32)
    got, exact = assign_candidates(val_h, idx_h, cnt_h, row0[:-1], q_per_frame, M, K_HI, K_LO, 4)
    redo = np.nonzero(~exact)[0]
    if ex.any_flag(len(redo) > 0, "cpu"):
        full = ex.gather_blocks(aug_local, M)[:len(q)].numpy()
        assert np.array_equal(full, full_rows(q)(0, M))        # the gathered blocks ARE the full rows
        for f in redo:
            a = np.ones((1, 7, M + 1), dtype=np.float16)
            a[0, :q_per_frame[f]] = full[row0[f]:row0[f + 1]]
            got[f] = assign_batch(a, [q_per_frame[f]], 4)[0]
    want_aug = full_rows(q)(0, M)
    for f in range(len(q_per_frame)):
        a = np.ones((1, 7, M + 1), dtype=np.float16)
        a[0, :q_per_frame[f]] = want_aug[row0[f]:row0[f + 1]]
        assert got[f] == assign_batch(a, [q_per_frame[f]], 4)[0], (rank, kind, f)
    if kind == "reid":
        assert exact.all(), "re-identification rows must be proved from the candidate lists"
    else:
        assert not exact.all()                           # the fall-back (flag all-reduce + block all-gather) ran on this rank
# the agreement collective at the start of a step: one rank's input error / end of batches is seen by every rank (ADVICE r2)
e, d, a = ex.agree(rank == 1, False, "cpu"); assert e and not d and a
e, d, a = ex.agree(False, rank == 0, "cpu"); assert not e and d and a           # one rank done, one active: both learn of the mismatch
e, d, a = ex.agree(False, True, "cpu"); assert not e and d and not a            # every rank done: a regular end
dist.barrier()
if rank == 0:
    print("TOPK_OK")
dist.destroy_process_group()
'''


def test_sharded_topk_allgather_gloo_world2(tmp_path):
    """SURVEY §8e / north star: memory embeddings sharded by instance range, per-shard two-ended top-k candidate lists all-gathered,
    exact assignment search on the merged lists (with the full-row fall-back agreed by all-reduce) == search on the full matrix"""
    script = tmp_path / "topk_worker.py"
    script.write_text(TOPK_WORKER)
    env = dict(os.environ, IBL_ROOT=ROOT, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                          "127.0.0.1", "--master-port", "29521", str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "TOPK_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
