"""CPU: the C-ABI library loads and exports every symbol include/ibloc.h declares (no compute calls)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    text = open(os.path.join(ROOT, "include", "ibloc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ibl_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from ibloc_amd import _lib
    names = declared_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(_lib.lib, n), f"{n} declared in include/ibloc.h but not exported by libibloc_hip.so"


def test_python_binding_covers_the_header():
    from ibloc_amd import _lib
    assert sorted(_lib.declared_symbols()) == declared_functions()


def test_error_channel_without_gpu():
    from ibloc_amd import _lib
    st = _lib.lib.ibl_assign_batch(None, None, 0, 0, 0, 0, None, None, None, 0, 0)
    assert st < 0 and b"null" in _lib.lib.ibl_last_error()


def test_registration_calls_refuse_null_arguments_without_gpu():
    """ibl_register_jobs and ibl_register_evaluate_batch with a null context, pool or params, and ibl_memgrid_build with a null context
    and reserve_points on an immutable grid: a negative status and a message, decided before any HIP call"""
    import numpy as np
    from ibloc_amd import _lib
    from ibloc_amd import registration as R
    lib, ref = _lib.lib, ctypes.byref
    seg = np.zeros(3, dtype=np.int32)
    one = np.zeros(16, dtype=np.float64)
    pool = R._PoolStruct(one.ctypes.data, seg.ctypes.data, seg.ctypes.data, None, 0)      # never dereferenced: every call below is refused
    params = R._ParamsStruct(0.05, 1.5, 0.4, 0, 1000, 0, 3)
    out = R._OutStruct(*([one.ctypes.data] * 7))
    ctx = ctypes.c_void_p(1)                                                              # non-null, never dereferenced either
    n_jobs, grid = ctypes.c_int32(0), ctypes.c_void_p()

    def refused(st):
        assert st < 0 and lib.ibl_last_error()

    for c, d, m, p in [(None, ref(pool), ref(pool), ref(params)), (ctx, None, ref(pool), ref(params)), (ctx, ref(pool), None, ref(params)),
                       (ctx, ref(pool), ref(pool), None)]:
        refused(lib.ibl_register_jobs(c, d, m, seg.ctypes.data, seg.ctypes.data, None, 1, p, ref(out), None))
        refused(lib.ibl_register_evaluate_batch(c, d, seg.ctypes.data, 0, seg.ctypes.data, seg.ctypes.data, seg.ctypes.data, 6, m, ctx, p,
                                                0.05, 8, 0.02, 1, seg.ctypes.data, ref(n_jobs), ref(out), one.ctypes.data, one.ctypes.data,
                                                one.ctypes.data, seg.ctypes.data, None))
    refused(lib.ibl_memgrid_build(None, one.ctypes.data, 4, 0.04, 0, 1, ref(grid), None))
    assert not grid


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    import importlib
    from ibloc_amd import _lib
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    try:
        _lib._load()
        assert False, "expected IblError"
    except _lib.IblError as e:
        assert "no CPU fallback" in str(e)


def test_struct_layouts_match_the_header(tmp_path):
    """the ctypes mirrors of the header's structs (ibloc_amd/vit.py, dator.py, siglip.py, preprocess.py, registration.py) have the sizes and the field
    offsets gcc gives the declarations of include/ibloc.h -- a drifted mirror would hand the library garbage pointers"""
    import subprocess
    from ibloc_amd import dator as D
    from ibloc_amd import preprocess as pp
    from ibloc_amd import registration as R
    from ibloc_amd import siglip as SG
    from ibloc_amd import vit as V
    pairs = [("ibl_vit_desc", V.VitDesc), ("ibl_vit_layer", V.VitLayer), ("ibl_vit_weights", V.VitWeights), ("ibl_linear_desc", V.LinearDesc),
             ("ibl_dator_head_weights", D.DatorHeadWeights), ("ibl_crop_desc", pp.CropDesc), ("ibl_instance_features", R._FeatStruct),
             ("ibl_cloud_pool", R._PoolStruct), ("ibl_register_params", R._ParamsStruct), ("ibl_register_out", R._OutStruct),
             ("ibl_probe_head_desc", SG.ProbeHeadDesc), ("ibl_probe_head_weights", SG.ProbeHeadWeights)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ibloc.h"', 'int main(void) {']
    for cname, ct in pairs:
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'  printf(" %zu", offsetof({cname}, {fname}));')
        lines.append('  printf("\\n");')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    for (cname, ct), line in zip(pairs, out):
        parts = line.split()
        assert parts[0] == cname
        assert int(parts[1]) == ctypes.sizeof(ct), f"sizeof({cname}) = {parts[1]}, ctypes mirror {ctypes.sizeof(ct)}"
        for (fname, _), off in zip(ct._fields_, parts[2:]):
            assert int(off) == getattr(ct, fname).offset, f"{cname}.{fname}: offset {off} in the header, {getattr(ct, fname).offset} in the mirror"


def test_constants_match_the_header(tmp_path):
    """the constants ibloc_amd/vit.py, dator.py and siglip.py mirror -- the descriptor flags, the epilogue, activation and LayerNorm-output
    enums, MAX_LAYERS, SPLIT_SCALE and the order of the three workspace-tap tuples -- have the values gcc gives include/ibloc.h's"""
    import subprocess
    from ibloc_amd import dator as D
    from ibloc_amd import siglip as SG
    from ibloc_amd import vit as V
    want = {"IBL_VIT_MAX_LAYERS": V.MAX_LAYERS, "IBL_VIT_SPLIT_SCALE": V.SPLIT_SCALE, "IBL_VIT_WS_COUNT": len(V.WS_TAPS),
            "IBL_DATOR_WS_COUNT": len(D.HEAD_TAPS), "IBL_PROBE_WS_COUNT": len(SG.HEAD_TAPS)}
    for name in ("LAYERSCALE", "PRE_LN", "FINAL_LN", "QUICK_GELU", "PROJ", "OUT_ALL_TOKENS", "ACT_TERMS2", "ACT_TERMS3", "NO_CLS", "TANH_GELU"):
        want["IBL_VIT_" + name] = getattr(V, "FLAG_" + name)
    for name in ("F16", "GELU_F16", "RESID_F32", "PATCH_F32", "F32", "RESID_PRE_F32", "GELU_F16_X2", "GELU_F16_X3"):
        want["IBL_LINEAR_" + name] = getattr(V, "LINEAR_" + name)
    for name in ("GELU_ERF", "QUICK_GELU", "GELU_TANH"):
        want["IBL_ACT_" + name] = getattr(V, "ACT_" + name)
    for name in ("F32", "F16", "F16_X2", "F16_X3"):
        want["IBL_LN_OUT_" + name] = getattr(V, "LN_" + name)
    for prefix, taps in (("IBL_VIT_WS_", V.WS_TAPS), ("IBL_DATOR_WS_", [n for n, _ in D.HEAD_TAPS]), ("IBL_PROBE_WS_", SG.HEAD_TAPS)):
        for i, name in enumerate(taps):
            want[prefix + name.upper()] = i
    lines = ['#include <stdio.h>', '#include "ibloc.h"', 'int main(void) {']
    lines += [f'  printf("{name} %.17g\\n", (double)({name}));' for name in want]
    lines += ['  return 0;', '}']
    src = tmp_path / "constants.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "constants"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[::2], map(float, out[1::2])))
    assert sorted(got) == sorted(want)
    for name, value in want.items():
        assert got[name] == value, f"{name}: {got[name]:g} in the header, {value} in the mirror"
    # every flag of the header is mirrored: a new IBL_VIT_* bit without a FLAG_* would be packed as 0
    header = open(os.path.join(ROOT, "include", "ibloc.h")).read()
    assert set(re.findall(r"#define\s+(IBL_VIT_[A-Z0-9_]+)\s", header)) == {n for n in want if n.startswith("IBL_VIT_") and "_WS_" not in n}
