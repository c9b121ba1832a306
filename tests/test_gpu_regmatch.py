"""-m gpu: feature matching alone (csrc/reg_match.hip + csrc/reg_featnn.hip) against the oracle, job by job, on the job sets of
tests/regmatch_cases.py (tests/test_regmatch_model.py shows on the CPU that every set is what it claims).  Crafted FPFH rows are
written into the instance features of both pools, so they decide the correspondence list; the geometry is laid out so that a
correspondence is an inlier exactly when it is the right answer (`instance_pair`), and `ransac_stats` / `T_ransac` -- the RANSAC
stage's own outputs, read back before ICP -- then pin content, order and length of the list: hypothesis i draws floor(r n_corr) from
the ordered list.  EVERY job's statistics equal the oracle's (`feature_match` on the job's concatenated rows, then `ransac`) and
|T_ransac - T_oracle| <= 1e-6 per entry; no tolerance on the statistics, no share of jobs that may miss.

Every family runs four ways, each compared with the ORACLE (not with another run): default (matrix cores, resident fp16 operands),
compact features (operands built from the fp32 rows while they are staged), `feat_valu=1` (the VALU scan), one job per call.  Status
bit 1 stays clear throughout, bits 16 / 32 (a call redone with the VALU search / a full survivor list) too: no run means to take a
fallback.  reuse[1] == 0 in every call: every row was served from the injected features.

family      path it exists for                                                                                    largest |T_ransac - T_oracle|
sizes       1 .. 600 rows against 1 .. 600: query tiles, 32-row chunks, the last partial chunk, nt < 32,          0
            the chunks pass 1 skips
ties        duplicated database / query rows inside a chunk, across chunks, across the pieces of 2- and           0
            3-piece sides; a tie between a non-mutual and a mutual target: lowest concatenated index
near_ties   distances d and d + 1 (d + 2^-12) with the farther row first, norms up to the domain's edge and       0
            rows fp16 does not hold: the filter passes both, the exact re-check chooses
crowded     queries with several hundred candidates: a wave's 256-entry queue flushes more than once              0
mutual      8 / 9 / 1 mutual pairs (fallback to all ns matches or not), ordered compaction over three             0
            256-blocks (one of them empty), short need lists, targets matched by many sources
pieces      2 and 3 instances per side, unequal sizes, an empty middle slot, pairs shared between jobs            0
(last column: the largest over the four ways.)  Measured on an MI355X: all 88 jobs agree in the three statistics in each of the four ways,
and every T_ransac is bit-identical to the oracle's.  No case had to be replaced.  The 24 runs take 0.5 s together; the slowest are
sizes / default (0.12 s) and sizes / single (64 calls, 0.05 s: the oracle's results are shared between the ways).
"""
import numpy as np
import pytest

from tests import regmatch_cases as rc

pytestmark = pytest.mark.gpu

TOL_T = 1e-6
WAYS = ("default", "compact", "valu", "single")


@pytest.fixture(scope="module")
def ctx():
    from ibloc_amd.registration import RegContext
    c = RegContext(4 << 30)
    yield c
    c.close()


def compare(name, fam, out, jobs=None):
    """every job against the oracle: statistics equal, T_ransac within TOL_T; returns the largest gap after asserting all jobs"""
    jobs = list(range(len(fam["js"]))) if jobs is None else list(jobs)
    want = [rc.expected(fam, j) for j in jobs]
    gaps = np.array([np.abs(out["T_ransac"][k] - w[1]).max() for k, w in enumerate(want)])
    missed = [(name, j, fam["tags"][j], len(want[k][0]), out["ransac_stats"][k].tolist(), want[k][2].tolist(), float(gaps[k]))
              for k, j in enumerate(jobs) if not (np.array_equal(out["ransac_stats"][k], want[k][2]) and gaps[k] <= TOL_T)]
    assert not missed, missed
    return gaps.max()


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("name", sorted(rc.FAMILIES))
def test_family(ctx, name, way):
    fam = rc.FAMILIES[name]()
    J = len(fam["js"])
    ctx.status()                                               # clear the sticky bits of earlier tests
    p = rc.pools(ctx, fam, compact=(way == "compact"))
    assert (p[2].fpfh_split is None) == (way == "compact") and (p[3].fpfh_split is None) == (way == "compact")
    if way == "single":
        worst = 0.0
        for j in range(J):
            out = rc.run(ctx, fam, p, jobs=[j])
            worst = max(worst, compare(name, fam, out, [j]))
    else:
        with ctx.diag(feat_valu=1 if way == "valu" else 0):
            out = rc.run(ctx, fam, p)
        worst = compare(name, fam, out)
        if name == "pieces":
            print("reuse", out["reuse"])
            assert out["reuse"][4] < out["reuse"][5]          # fewer distinct (query instance, database instance) searches than uses
    st = ctx.status()
    assert st & (1 | 16 | 32) == 0, st                        # no grid overflow, no call redone: the paths named above were the ones taken
    print(f"{name} / {way}: {J} jobs, largest gap in T_ransac {worst:.2e}")


def test_operand_builder_reproduces_the_librarys_operands_bit_for_bit(ctx):
    """the numpy restatement of fm_centred_norm / fm_operand_piece that `inject` writes crafted rows with, on REAL rows: from the library's
    own fpfh of SynthWorld clouds of a few hundred points it gives the library's fpfh_norm and fpfh_split, every bit"""
    import torch
    from ibloc_amd.registration import CloudBatch, instance_features_batch
    from ibloc_amd.synth import SynthWorld
    w = SynthWorld(4, pts_per_object=300, E=1, D=8, seed=71)
    mem = CloudBatch.from_numpy(w.points)
    ft = instance_features_batch(ctx, mem, rc.VOXEL, grad_radius=rc.GRAD_RADIUS)
    torch.cuda.synchronize()
    stored = ft.fpfh[:mem.n].cpu().numpy()
    assert len(stored) >= 1000 and stored.max() > 50 and len(np.unique(stored)) > 1000          # real histograms, full mantissas
    norm = rc.centred_norm(stored)
    assert np.array_equal(norm.view(np.uint32), ft.fpfh_norm[:mem.n].cpu().numpy().view(np.uint32))
    op = rc.operand_rows(stored, norm)
    assert np.array_equal(op.view(np.uint16), ft.fpfh_split[:mem.n].view(torch.int16).cpu().numpy().view(np.uint16))
