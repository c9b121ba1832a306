"""CPU: the stage machinery of tests/vit_stream_cases.py on trained-LIKE weight statistics (tests/vit_trained_cases.py), with the
references alone.

For every family x kind x plan (`plain`, `p2;*:3333`, `p2;0:3232;1:2211;2:2111`):
  (a) the fp32 stand-in for the device stays inside every stage bound and the 2 % cap, exactly as in tests/test_vit_stream_model.py
      (no bound, cap or constant of a `*_cases.py` formula is changed for these weights);
  (b) on kind `all`, every mutant of MUTANTS that applies is still refused (`p2;*:2222`, `p2;*:3333`);
  (c) the kinds are what they claim, measured on the fp64 forward, and none of them reaches the fp16 clamp;
  (d) the end-to-end yardstick of tests/test_gpu_vit_trained.py: the chained emulation (fp64 accumulation) and the chained stand-in (fp32)
      against oracle/vit_oracle.vit_forward in float64; R = max err_standin / err_emu is printed, and E2E_MARGIN >= 1.25 R is asserted
      row by row."""
import functools

import numpy as np
import pytest
import torch

from oracle import vit_oracle as vo
from tests import vit_stream_cases as SCS
from tests import vit_trained_cases as TC

CASES = [(f, k, p) for f in SCS.FAMILIES for k in TC.kinds_of(f) for p in TC.PLANS]
MUTANT_PLANS = ("p2;*:2222", "p2;*:3333")


def _id(c):
    return "-".join(c)


@functools.lru_cache(maxsize=None)
def chain(family, kind, plan):
    """test_vit_stream_model.chain on the weights of `kind`"""
    m = SCS.Model(family, plan, kind=kind)
    x0 = SCS.stage_patch(m, np.float32)["emu"]
    xs, full, cls = [x0], [], []
    for l in range(SCS.DEPTH):
        full.append(SCS.stand_in(m, l, xs[-1]))
        if m.cfg.cls_token:
            cls.append(SCS.stand_in(m, l, xs[-1], cls_only=True))
        xs.append(full[-1]["x"])
    return m, xs, full, cls


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_fp32_stand_in_stays_inside_cap_and_bound(case):
    m, xs, full, cls = chain(*case)
    r, ok = SCS.check32("patch", xs[0], SCS.stage_patch(m))
    assert ok, f"patch: {r:.3f}"
    for l in range(SCS.DEPTH):
        for cls_only, dev in ((False, full[l]),) + (((True, cls[l]),) if cls else ()):
            for stage, ratio, share, ok in SCS.block_checks(m, l, xs[l], dev, cls_only=cls_only):
                print(f"{_id(case)} block {l} {'cls ' if cls_only else ''}{stage}: ratio {ratio:.3f}" + ("" if share is None else f" unequal {share:.4%}"))
                assert ok, (l, cls_only, stage, ratio, share)
    x_cls = np.ascontiguousarray(xs[-1][::m.T])
    if m.cfg.proj_dim:
        ln, proj = SCS.stage_out_proj(m, x_cls)
        assert SCS.check16("out_ln", ln["emu"], ln, m.D)[2]
        assert SCS.check32("out_proj", proj(ln["emu"])["emu"].astype(np.float32), proj(ln["emu"]))[1]
        got = SCS.stage_out_proj(m, x_cls, np.float32)[1](ln["emu"])["emu"]
        assert SCS.check32("out_proj", got, proj(ln["emu"]))[1]
    st = SCS.stage_out_ln(m, xs[-1])
    assert SCS.check32("out_ln32", st["emu"], st)[1]


def _mutant_cases():
    out = []
    for family in SCS.FAMILIES:
        for plan in MUTANT_PLANS:
            m = SCS.Model(family, plan, kind="all")
            for mutant in SCS.MUTANTS:
                if SCS.applies(mutant, m, "patch"):
                    out.append((family, plan, mutant, "patch", 0, False))
                if SCS.applies(mutant, m, "proj") and m.cfg.proj_dim:
                    out.append((family, plan, mutant, "proj", 0, False))
                for l in range(SCS.DEPTH):
                    for cls_only in (False, True) if m.cfg.cls_token else (False,):
                        for stage in ("qkv", "att", "ln2", "hid", "resid"):
                            if SCS.applies(mutant, m, stage, l, cls_only):
                                out.append((family, plan, mutant, stage, l, cls_only))
    return out


MUTANT_CASES = _mutant_cases()


def test_every_mutant_has_cases():
    assert {c[2] for c in MUTANT_CASES} == set(SCS.MUTANTS)


@pytest.mark.parametrize("case", MUTANT_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-{c[3]}{c[4]}{'-cls' if c[5] else ''}")
def test_a_mutant_as_the_reference_is_refused(case):
    """kind `all`: the stand-in (a correct chain) against the reference with one mutation must leave the cap or the bound at that stage"""
    family, plan, mutant, stage, l, cls_only = case
    m, xs, full, cls = chain(family, "all", plan)
    if stage == "patch":
        r, ok = SCS.check32("mutant", xs[0], SCS.stage_patch(m, mutant=mutant))
        assert not ok, f"patch {mutant}: ratio {r:.3f}"
        return
    if stage == "proj":
        x_cls = np.ascontiguousarray(xs[-1][::m.T])
        ln, _ = SCS.stage_out_proj(m, x_cls)
        got = SCS.stage_out_proj(m, x_cls, np.float32)[1](ln["emu"])["emu"]
        r, ok = SCS.check32("mutant", got, SCS.stage_out_proj(m, x_cls, mutant=mutant)[1](ln["emu"]))
        assert not ok, f"proj {mutant}: ratio {r:.3f}"
        return
    dev = (cls if cls_only else full)[l]
    saved = {k: list(v) for k, v in SCS.WORST.items()}
    res = SCS.block_checks(m, l, xs[l], dev, mutant=mutant, cls_only=cls_only, stages=(stage,))
    SCS.WORST.clear()
    SCS.WORST.update(saved)
    assert res and not all(ok for _, _, _, ok in res), f"{stage} {mutant}: {res}"


# ---- (c) the kinds are what they claim -------------------------------------------------------------------------------------------------
def test_random_is_todays_weights_and_kinds_are_deterministic():
    from ibloc_amd import vit as V
    for i, family in enumerate(SCS.FAMILIES):
        cfg, w, px = SCS.inputs(family)
        assert SCS.inputs(family, "random") is not None and SCS.Model(family, "plain").w is SCS.Model(family, "plain", kind="random").w
        ref = V.random_weights(cfg, SCS.WSEED + i)
        assert set(w) == set(ref) - ({"patch.b"} if family == "clip" else set())
        assert all(np.array_equal(w[k], ref[k]) for k in w)
        for kind in TC.kinds_of(family):
            a, b = TC.trained_like(cfg, w, TC.SEED + i, kind), TC.trained_like(cfg, w, TC.SEED + i, kind)
            assert set(a) == set(w) and all(np.array_equal(a[k], b[k]) and a[k].dtype == np.float32 for k in a)
            assert all(np.array_equal(a[k], SCS.inputs(family, kind)[1][k]) for k in a)
            assert any(not np.array_equal(a[k], w[k]) for k in a), (family, kind)
            assert all(np.array_equal(w[k], ref[k]) for k in w), "trained_like changed its input"


@pytest.mark.parametrize("family", list(SCS.FAMILIES))
def test_forward64_is_the_oracle_in_double(family):
    """the fp64 forward the statistics are measured on equals oracle/vit_oracle.vit_forward(dtype=float64) on every token after the
    blocks (to the rounding of double: the two differ in the order of sums and in eps rounded to fp32)"""
    import dataclasses
    for kind in ("random", "all"):
        cfg, w, px = SCS.inputs(family, kind)
        ref = vo.vit_forward(w, dataclasses.replace(cfg, final_ln=False, proj_dim=0), px, all_tokens=True, dtype=torch.float64)
        got = TC.forward64(family, kind)["x"][-1]
        assert TC.rel_l2(got, ref.reshape(got.shape)) < 1e-7


@pytest.mark.parametrize("family", list(SCS.FAMILIES))
def test_kinds_are_what_they_claim(family):
    cfg = SCS.FAMILIES[family]
    sub_any = 0.0
    for kind in ("random",) + TC.kinds_of(family):
        r = TC.forward64(family, kind)
        w = SCS.inputs(family, kind)[1]
        x1 = np.abs(r["x"][1])
        massive = float(x1.max() / np.median(x1))
        peak = float(np.mean([p.max(axis=-1).mean() for p in r["probs"]]))
        ls = float(np.median(np.abs(np.concatenate([w[f"l{l}.{n}"] for l in range(cfg.depth) for n in ("ls1", "ls2")])))) if cfg.layerscale else float("nan")
        gains = [np.abs(w[n + ".g"]) for n in TC._ln_names(cfg, w)]
        gain = float(min(g.max() / np.median(g) for g in gains))
        top = {b: float(max(np.abs(a).max() for a in r[b])) for b in ("qkv", "att", "xn1", "xn", "hid")}
        sub = {b: float(np.mean([TC.subnormal_share(a) for a in r[b]])) for b in ("xn1", "att", "xn", "hid")}
        print(f"{family:>6} {kind:>8}: max|x|/median|x| into block 1 {massive:8.1f}, mean top probability {peak:.3f}, median|ls| {ls:.4f}, "
              f"min over LNs of max|g|/median|g| {gain:6.2f}, largest fp16 |ref| " + " ".join(f"{b} {v:.1f}" for b, v in top.items()) +
              ", fp16-subnormal share of a / S " + " ".join(f"{b} {v:.3%}" for b, v in sub.items()))
        if kind in ("massive", "all"):
            assert massive >= 100, (family, kind, massive)
        # (not asserted on `all`: massive channels take most of a row's variance, so LayerNorm 1 hands q and k smaller rows and the logits
        # narrow again -- vit: 0.57.  The figure is printed)
        if kind == "peaked":
            assert peak >= 0.8, (family, kind, peak)
        if kind in ("small_ls", "all") and cfg.layerscale:
            assert ls <= 0.1, (family, kind, ls)
        if kind in ("ln_heavy", "all"):
            assert gain >= 8, (family, kind, gain)
        assert max(top.values()) < 65504 / 4, (family, kind, top)       # these tests are about rounding, not about the clamp
        if kind != "random":
            sub_any = max(sub_any, max(sub.values()))
    assert sub_any > 0, "no kind puts an element of an a / S block into the fp16 subnormals"


# ---- (d) the end-to-end yardstick ------------------------------------------------------------------------------------------------------
RATIOS = {}


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_end_to_end_yardstick(case):
    family, kind, plan = case
    ref = TC.reference_out(family, kind)
    e_emu = TC.err_emu(family, kind, plan)
    m, xs, full, cls = chain(*case)         # the stand-in of (a): its last block CLS-only where there is a class token, as the device runs it
    e_std = TC.rel_l2(TC.chain_end(m, cls[-1]["x"] if cls else xs[-1], np.float32), ref)
    RATIOS[case] = e_std / e_emu
    print(f"{_id(case)}: err_emu {e_emu:.3e} err_standin {e_std:.3e} ratio {e_std / e_emu:.3f}")
    assert np.isfinite(e_emu) and e_emu > 0
    assert e_std <= TC.E2E_MARGIN * e_emu, (case, e_std, e_emu)


def test_zz_margin_is_the_measured_ratio():
    """prints R over the table above; E2E_MARGIN is 1.25 R rounded up to one decimal (when the whole table ran)"""
    if not RATIOS:              # (run on its own: nothing to compare)
        return
    worst = max(RATIOS, key=RATIOS.get)
    R = RATIOS[worst]
    print(f"R = {R:.3f} at {_id(worst)} over {len(RATIOS)} rows; 1.25 R = {1.25 * R:.3f}; E2E_MARGIN = {TC.E2E_MARGIN}")
    if len(RATIOS) == len(CASES):
        assert TC.E2E_MARGIN == np.ceil(1.25 * R * 10 - 1e-9) / 10, (R, TC.E2E_MARGIN)
