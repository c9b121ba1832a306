"""-m gpu: the diagnostic switches of a registration context (include/ibloc.h at ibl_reg_ctx_set_diag): defaults, refusals, clamps,
the environment read once at creation, RegContext.diag() restoring what it found, and switches of one context leaving another alone.
(A context can only be created on a device; no test here launches more than one small registration.)"""
import os
import re

import numpy as np
import pytest

from ibloc_amd.synth import SynthWorld

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ("knn_noguess", "knn_debug", "feat_unfused", "feat_valu", "feat_cand_cap", "spfh_f64", "spfh_qcap", "spfh_stats", "eval_fullscan",
         "timing")
NAMES = ("knn_safety", "knn_rho", "feat_p1_stride") + FLAGS


def defaults():
    src = open(os.path.join(ROOT, "instance-based-loc_amd", "csrc", "reg_common.h")).read()
    stride = int(re.search(r"^#define FM_P1_STRIDE (\d+)", src, flags=re.M).group(1))          # the library's constant
    return dict({n: 0.0 for n in FLAGS}, knn_safety=1.1, knn_rho=3.0, feat_p1_stride=float(stride))


@pytest.fixture()
def clean_env(monkeypatch):
    for n in NAMES:
        monkeypatch.delenv("IBL_" + n.upper(), raising=False)
    return monkeypatch


@pytest.fixture()
def ctx(clean_env):
    from ibloc_amd.registration import RegContext
    c = RegContext(1 << 20)
    yield c
    c.close()


def test_a_fresh_context_reports_the_defaults(ctx):
    assert {n: ctx.diag_get(n) for n in NAMES} == defaults()


def test_unknown_name_nan_and_null_name_are_refused_and_change_nothing(ctx):
    from ibloc_amd._lib import IblError
    for bad in (lambda: ctx.diag_set("no_such_switch", 1), lambda: ctx.diag_get("no_such_switch"),
                lambda: ctx.diag_set("knn_rho", float("nan")), lambda: ctx.diag_set("spfh_qcap", float("inf")),
                lambda: ctx.diag_set(None, 1), lambda: ctx.diag_get(None)):
        with pytest.raises(IblError):
            bad()
    with pytest.raises(IblError):
        with ctx.diag(knn_noguess=1, no_such_switch=1):
            pass
    with pytest.raises(IblError):
        with ctx.diag(knn_noguess=1, knn_rho=float("nan")):
            pass
    assert {n: ctx.diag_get(n) for n in NAMES} == defaults()


def test_the_setter_clamps(ctx):
    ctx.diag_set("knn_rho", 9)
    assert ctx.diag_get("knn_rho") == 4
    ctx.diag_set("knn_rho", -3)
    assert ctx.diag_get("knn_rho") == 1
    for cap in ("spfh_qcap", "feat_cand_cap"):
        ctx.diag_set(cap, -5)
        assert ctx.diag_get(cap) == 1
        ctx.diag_set(cap, 0)
        assert ctx.diag_get(cap) == 0                   # 0 = sized by the call
    ctx.diag_set("feat_p1_stride", 0)
    assert ctx.diag_get("feat_p1_stride") == 1          # (a stride of 0 would never advance)
    ctx.diag_set("knn_safety", 0.8)
    assert ctx.diag_get("knn_safety") == 0.8


def test_the_environment_is_read_at_creation_only_and_per_context(clean_env):
    from ibloc_amd.registration import RegContext
    a = RegContext(1 << 20)
    clean_env.setenv("IBL_SPFH_QCAP", "8")
    clean_env.setenv("IBL_FEAT_VALU", "0")              # every switch is a number: 0 is off
    b = RegContext(1 << 20)
    assert b.diag_get("spfh_qcap") == 8 and a.diag_get("spfh_qcap") == 0
    assert b.diag_get("feat_valu") == 0
    clean_env.delenv("IBL_SPFH_QCAP")
    assert b.diag_get("spfh_qcap") == 8 and a.diag_get("spfh_qcap") == 0
    a.close()
    b.close()


def test_diag_restores_what_it_found_also_when_the_body_raises(ctx, clean_env):
    from ibloc_amd.registration import RegContext
    with pytest.raises(ZeroDivisionError):
        with ctx.diag(knn_noguess=1, spfh_qcap=8):
            assert ctx.diag_get("knn_noguess") == 1 and ctx.diag_get("spfh_qcap") == 8
            1 / 0
    assert ctx.diag_get("knn_noguess") == 0 and ctx.diag_get("spfh_qcap") == 0
    clean_env.setenv("IBL_KNN_RHO", "2")
    c = RegContext(1 << 20)
    with c.diag(knn_rho=4):
        assert c.diag_get("knn_rho") == 4
    assert c.diag_get("knn_rho") == 2                   # what the context had, not the library's default 3
    c.close()


def test_a_switch_of_one_context_leaves_another_context_alone(clean_env):
    """the same registration in two contexts: A with a 100-entry candidate list (the matrix-core search overflows, the call is redone
    with the VALU search: status bit 4), B untouched (no redo), equal results bit for bit"""
    from ibloc_amd.registration import CloudBatch, RegContext, instance_features_batch, register_batch
    from oracle import reg_oracle as ro
    w = SynthWorld(4, pts_per_object=1500, E=1, D=8, seed=61)
    f = w.make_frame(np.random.default_rng(62), q=3, pts_per_object=1500, anchor=1)
    ids = f["ids"]
    det = CloudBatch.from_numpy([c[0] for c in f["clouds"]], [ro.intensity(c[1]) for c in f["clouds"]])
    mem = CloudBatch.from_numpy(w.points, [ro.intensity(c) for c in w.colors])
    js, jt = [[0, -1, -1], [1, 2, -1]], [[ids[0], -1, -1], [ids[1], ids[2], -1]]
    a, b = RegContext(1 << 30), RegContext(1 << 30)
    fd = instance_features_batch(a, det, 0.05)
    fm = instance_features_batch(a, mem, 0.05, grad_radius=0.15)
    with a.diag(feat_cand_cap=100):
        out_a = register_batch(a, det, mem, js, jt, 0.05, 1.5, 1.5, seed=3, job_id_base=40, det_features=fd, mem_features=fm)
    st_a = a.status()
    out_b = register_batch(b, det, mem, js, jt, 0.05, 1.5, 1.5, seed=3, job_id_base=40, det_features=fd, mem_features=fm)
    st_b = b.status()
    assert st_a & 16 == 16 and st_b & 16 == 0, (st_a, st_b)
    for k in ("T", "rmse", "fitness", "T_ransac", "ransac_stats", "means"):
        assert np.array_equal(out_a[k], out_b[k]), k
    a.close()
    b.close()
