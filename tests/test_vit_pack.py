"""CPU: the host's packing decision (ibloc_amd/vit.py `plan_terms`, `pack_top`, `pack_layer`, `validate`, `make_desc`) against the
independent restatement of tests/vit_stream_cases.py -- `Model.terms` / `lo_launch` / `layer`, `w_terms`, `w_lo` -- on its four families,
four plans and `EXTRA` (launch-per-term, folded LayerScale) at n_blocks_run = DEPTH, all tokens and class rows.  Bit for bit: the arrays
tagged fp16 are rounded with `SCS.f16` and compared as uint16, the fp32 ones as float32 bits; and a field a block does not use must be
absent, which no forward can see."""
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest

from ibloc_amd import vit as V
from tests import vit_stream_cases as SCS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(f, p, True, False) for f in SCS.FAMILIES for p in SCS.PLANS] + SCS.EXTRA
# without a class token there are no class rows to return (`validate` refuses it)
RUNS = [c + (all_tokens,) for c in CASES for all_tokens in ((True, False) if SCS.FAMILIES[c[0]].cls_token else (True,))]


def run_id(r):
    f, p, kext, fold, all_tokens = r
    return f"{f}-{p}" + ("" if kext else "-kext0") + ("-fold" if fold else "") + ("-all" if all_tokens else "-cls")


def setup(run):
    family, plan, kext, fold, all_tokens = run
    m = SCS.Model(family, plan, kext, fold)
    cfg = SCS.run_cfg(family, SCS.DEPTH, all_tokens)
    patch_terms, layer_terms = V.parse_precision(plan)
    return m, cfg, patch_terms, V.plan_terms(cfg, layer_terms, kext)


def cls_only(run, l):
    return not run[4] and l == SCS.DEPTH - 1


def same(packed, want16, want32):
    """packed {field: (tag, float32 array)} holds exactly the fields of want16 (fp16 arrays) and want32 (fp32 arrays), bit for bit"""
    assert set(packed) == set(want16) | set(want32), sorted(set(packed) ^ (set(want16) | set(want32)))
    for name, (tag, a) in packed.items():
        a = np.ascontiguousarray(a, dtype=np.float32)
        if name in want16:
            assert tag == V.F16, name
            want = want16[name]
            assert a.shape == want.shape and np.array_equal(SCS.f16(a).view(np.uint16), want.view(np.uint16)), name
        else:
            assert tag == V.F32, name
            want = np.ascontiguousarray(want32[name], dtype=np.float32)
            assert a.shape == want.shape and np.array_equal(a.view(np.uint32), want.view(np.uint32)), name


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_plan(run):
    m, cfg, _, (terms, lo_launch, act_terms) = setup(run)
    assert len(terms) == len(lo_launch) == cfg.depth
    for l in range(cfg.depth):
        assert tuple(terms[l]) == tuple(m.terms(l, cls_only(run, l))), l
        assert tuple(lo_launch[l]) == tuple(m.lo_launch(l, cls_only(run, l))), l
    resid = [t for l in range(cfg.depth) for t in m.terms(l, cls_only(run, l))[1::2]]         # the o and fc2 terms of every block
    assert act_terms == (max(resid) if run[2] else 1)


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_layers_bit_for_bit(run):
    m, cfg, _, (terms, lo_launch, _) = setup(run)
    S = np.float32(SCS.S)
    for l in range(cfg.depth):
        L = m.layer(l)
        qt, ot, ft, f2t = m.terms(l, cls_only(run, l))
        lo_o, lo_f = m.lo_launch(l, cls_only(run, l))
        w16 = {"w_qkv": SCS.w_terms(L["wqkv"], 1), "w_o": SCS.w_terms(L["wo"], 1), "w_fc1": SCS.w_terms(L["w1"], 1), "w_fc2": SCS.w_terms(L["w2"], 1)}
        w32 = {"ln1_g": L["g1"], "ln1_b": L["b1"], "b_qkv": L["bqkv"], "b_o": L["bo"], "ln2_g": L["g2"], "ln2_b": L["b2"], "b_fc1": L["bb1"],
               "b_fc2": L["bb2"]}
        ints = {}
        for field, w, t in (("qkv", L["wqkv"], qt), ("o", L["wo"], ot), ("fc1", L["w1"], ft), ("fc2", L["w2"], f2t)):
            if t > 1:
                w16[f"w_{field}_x"], ints[f"{field}_terms"] = SCS.w_terms(w, t), t
        for i, (field, w, lo) in enumerate((("o", L["wo"], lo_o), ("fc2", L["w2"], lo_f)), start=1):
            ls = L[f"ls{i}"]
            if ls is not None:                      # (None: no LayerScale, or folded into the weights and the bias)
                w32[f"ls{i}"] = ls
            if lo:
                w16[f"w_{field}_lo"] = SCS.w_lo(w)
                if not m.fold:
                    w32[f"ls{i}_lo"] = (ls if ls is not None else np.ones(m.D, np.float32)) / S
        fields = list(V.pack_layer(cfg, m.w, l, terms[l], lo_launch[l], m.fold))
        assert len({n for n, _ in fields}) == len(fields), "a field is packed twice"
        packed, got_ints = {n: v for n, v in fields if not isinstance(v, int)}, {n: v for n, v in fields if isinstance(v, int)}
        same(packed, w16, w32)
        assert got_ints == ints, l
        if cls_only(run, l):                        # nothing beyond the plain fields
            assert not got_ints and not [n for n in packed if n.endswith(("_x", "_lo"))]


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_top_bit_for_bit(run):
    m, cfg, patch_terms, _ = setup(run)
    w, plan = m.w, run[1]
    wp = np.zeros((cfg.dim, cfg.patch_k_pad), np.float32)
    wp[:, :cfg.patch_k] = w["patch.w"].reshape(cfg.dim, -1)
    pos = np.asarray(w["pos"], np.float32)                 # the families store the table of their run grid: used as stored
    w16 = {"w_patch": SCS.f16(wp)}
    w32 = {"pos_patch": pos[1:] if cfg.cls_token else pos}
    if patch_terms == 2:
        w16["w_patch_lo"] = SCS.w_lo(wp)
    if "patch.b" in w:
        w32["b_patch"] = w["patch.b"]
    if cfg.cls_token:
        w32["cls_pos"] = np.asarray(w["cls"], np.float32).reshape(-1) + pos[0]
    if cfg.pre_ln:
        w32["ln_pre_g"], w32["ln_pre_b"] = w["ln_pre.g"], w["ln_pre.b"]
    if cfg.final_ln:
        w32["ln_f_g"], w32["ln_f_b"] = w["ln_f.g"], w["ln_f.b"]
    if cfg.proj_dim:
        w16["w_proj"] = SCS.w_terms(w["proj.w"], 1)
        if plan != "plain":
            w16["w_proj_x"] = SCS.w_terms(w["proj.w"], 3)
    same(V.pack_top(cfg, w, patch_terms, proj_x=plan != "plain"), w16, w32)


def test_registers_and_rope_fields():
    """the fields no stream family has: register rows as stored, the rotary table, zeros for the position rows of a rotary model"""
    cfg = V.CONFIGS["tiny_dinov3"]
    w = V.random_weights(cfg, 3)
    a = V.pack_top(cfg, w)
    assert a["reg_tokens"][0] == V.F32 and np.array_equal(a["reg_tokens"][1], w["reg"])
    assert np.array_equal(a["rope_table"][1], V.rope_table(cfg.grid[0], cfg.grid[1], cfg.rope_theta))
    assert a["pos_patch"][1].shape == (cfg.n_patches, cfg.dim) and not a["pos_patch"][1].any()
    assert np.array_equal(a["cls_pos"][1], w["cls"])
    assert "w_patch_lo" not in a and "w_proj" not in a and "ln_pre_g" not in a


# ---- refusals: every ValueError of the constructor, raised by the pure functions -------------------------------------------------------------
def _tiny(name="tiny_dino", **kw):
    cfg = dataclasses.replace(V.CONFIGS[name], **kw)
    return cfg, V.random_weights(V.CONFIGS[name], 5)


def _refusals():
    both = _tiny("tiny_clip", quick_gelu=True, tanh_gelu=True)
    head_dim = _tiny(heads=4)
    reg_missing = _tiny(n_registers=4)
    reg_extra = (V.CONFIGS["tiny_dino"], V.random_weights(V.CONFIGS["tiny_dino_reg"], 5))
    reg_no_cls = _tiny("tiny_siglip", n_registers=4)
    rope_pos = (V.CONFIGS["tiny_dinov3"], dict(V.random_weights(V.CONFIGS["tiny_dinov3"], 5), pos=np.zeros((197, 128), np.float32)))
    no_cls_rows = _tiny("tiny_siglip", out_all_tokens=False)
    other_grid = (V.CONFIGS["tiny_siglip_384"], V.random_weights(V.CONFIGS["tiny_siglip"], 5))
    other_grid_cfg = _tiny("tiny_siglip", pos_grid=(24, 24))
    deep = _tiny(depth=V.MAX_LAYERS + 1)
    yield "both GELUs", both, "quick_gelu and tanh_gelu are both set"
    yield "head_dim", head_dim, "head_dim 32 is not supported: the attention and rotation kernels run head_dim 64"
    yield "registers missing", reg_missing, r"the weights hold registers of shape \(0,\), the configuration tiny_dino needs \(4, 128\)"
    yield "registers not wanted", reg_extra, "the weights hold 4 register tokens, the configuration tiny_dino none"
    yield "registers without a class row", reg_no_cls, "n_registers needs cls_token: registers follow the class row"
    yield "rope and pos", rope_pos, "rope_theta and a position table are both given"
    yield "no class row to return", no_cls_rows, "cls_token=False needs out_all_tokens: there is no class row to return"
    yield "table of another grid", other_grid, r"cls_token=False: the position table \(196, 128\) of grid \(24, 24\) must be that of the run grid \(24, 24\)"
    yield "grid of another table", other_grid_cfg, r"cls_token=False: the position table \(196, 128\) of grid \(24, 24\) must be that of the run grid \(14, 14\)"
    yield "too many layers", deep, "too many layers"


REFUSALS = list(_refusals())


@pytest.fixture
def no_upload(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("an upload before the refusal")
    monkeypatch.setattr(V.VitEncoder, "_upload", refuse)


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_configurations(case, no_upload):
    _, (cfg, w), message = case
    with pytest.raises(ValueError, match=message):
        V.validate(cfg, w)
    with pytest.raises(ValueError, match=message):
        V.pack_top(cfg, w)
    with pytest.raises(ValueError, match=message):
        V.VitEncoder(cfg, w, device="cpu", precision="plain")


@pytest.mark.parametrize("plan,message", [("p2;*:2322", "o = 3 needs the K-extended form"), ("p2;0:2223", "fc2 = 3 needs the K-extended form")])
def test_three_terms_refused_without_kext(plan, message, no_upload):
    cfg, w = _tiny()
    layer_terms = V.parse_precision(plan)[1]
    with pytest.raises(ValueError, match=message):
        V.plan_terms(cfg, layer_terms, False)
    V.plan_terms(cfg, layer_terms, True)
    with pytest.raises(ValueError, match=message):
        V.VitEncoder(cfg, w, device="cpu", precision=plan, resid_kext=False)
    # the class-rows-only last block stays plain, so its entry is not read
    V.plan_terms(cfg, V.parse_precision("1:2323")[1], False)


@pytest.mark.parametrize("plan,message", [("p3", "patch terms: 1 or 2"), ("0:222", "bad precision entry '0:222'"),
                                          ("0:2242", "bad precision entry '0:2242'"), ("p2;*:2022", "bad precision entry")])
def test_bad_plan_strings(plan, message, no_upload):
    with pytest.raises(ValueError, match=message):
        V.parse_precision(plan)
    with pytest.raises(ValueError, match=message):
        V.VitEncoder(*_tiny(), device="cpu", precision=plan)


# ---- options -----------------------------------------------------------------------------------------------------------------------------------
def test_options_are_resolved_once(monkeypatch):
    for name in ("IBL_VIT_PREC", "IBL_VIT_FOLD_LS", "IBL_VIT_RESID_KEXT"):
        monkeypatch.delenv(name, raising=False)
    assert V.resolve_options("p2;*:3333") == ("p2;*:3333", False, True)
    monkeypatch.setenv("IBL_VIT_PREC", "plain")
    monkeypatch.setenv("IBL_VIT_FOLD_LS", "1")
    monkeypatch.setenv("IBL_VIT_RESID_KEXT", "0")
    assert V.resolve_options("p2;*:3333") == ("plain", True, False)
    assert V.resolve_options("p2;*:3333", "p2", False, True) == ("p2", False, True)       # arguments win over the environment
    cfg, w = _tiny()
    enc = V.VitEncoder(cfg, w, device="cpu", precision="p2;*:2222")
    assert (enc.precision, enc.fold_layerscale, enc.act_terms) == ("p2;*:2222", True, 1) and enc.W.layers[0].w_o_lo and not enc.W.layers[0].w_o_x
    enc = V.VitEncoder(cfg, w, device="cpu", precision="p2;*:2222", fold_layerscale=False, resid_kext=True)
    assert (enc.fold_layerscale, enc.act_terms) == (False, 2) and enc.W.layers[0].w_o_x and not enc.W.layers[0].w_o_lo
    src = open(os.path.join(ROOT, "instance-based-loc_amd", "vit.py")).read() + open(os.path.join(ROOT, "instance-based-loc_amd", "dator.py")).read() \
        + open(os.path.join(ROOT, "instance-based-loc_amd", "siglip.py")).read()
    reads = len(re.findall(r"os\.environ|getenv", inspect.getsource(V.resolve_options)))
    assert reads == 3 and len(re.findall(r"os\.environ|getenv", src)) == reads, "the environment is read in resolve_options and nowhere else"


# ---- descriptor flags ------------------------------------------------------------------------------------------------------------------------
def header_defines():
    text = open(os.path.join(ROOT, "include", "ibloc.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+IBL_VIT_([A-Z0-9_]+)\s+(\d+)\s", text)}


TINY_FLAGS = {
    "tiny_dino": ("LAYERSCALE", "FINAL_LN"), "tiny_dino_518": ("LAYERSCALE", "FINAL_LN"),
    "tiny_clip": ("PRE_LN", "FINAL_LN", "PROJ"), "tiny_clip_q": ("PRE_LN", "FINAL_LN", "PROJ", "QUICK_GELU"),
    "tiny_siglip": ("FINAL_LN", "OUT_ALL_TOKENS", "NO_CLS", "TANH_GELU"), "tiny_siglip_384": ("FINAL_LN", "OUT_ALL_TOKENS", "NO_CLS", "TANH_GELU"),
    "tiny_dino_reg": ("LAYERSCALE", "FINAL_LN"), "tiny_dino_reg_518": ("LAYERSCALE", "FINAL_LN"),
    "tiny_dinov3": ("LAYERSCALE", "FINAL_LN"), "tiny_dinov3_384": ("LAYERSCALE", "FINAL_LN"),
}


def test_descriptor_flags():
    H = header_defines()
    assert sorted(TINY_FLAGS) == sorted(n for n in V.CONFIGS if n.startswith("tiny_"))
    for name, flags in TINY_FLAGS.items():
        cfg = V.CONFIGS[name]
        base = 0
        for f in flags:
            base |= H[f]
        for act_terms, extra in ((1, 0), (2, H["ACT_TERMS2"]), (3, H["ACT_TERMS3"])):
            d = V.make_desc(cfg, act_terms)
            assert d.flags == base | extra, (name, act_terms, d.flags)
        assert (d.n_blocks_run, d.n_tokens, d.out_dim, d.n_registers) == (cfg.depth, cfg.n_tokens, cfg.out_dim, cfg.n_registers)
    # all tokens of a DINOv2 trunk, one block short: the two descriptor fields no tiny configuration sets
    d = V.make_desc(dataclasses.replace(V.CONFIGS["tiny_dino"], out_all_tokens=True, n_blocks_run=1))
    assert d.flags == H["LAYERSCALE"] | H["FINAL_LN"] | H["OUT_ALL_TOKENS"] and d.n_blocks_run == 1
