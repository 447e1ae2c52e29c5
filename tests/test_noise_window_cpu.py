"""CPU suite for the resident frame windows with a noise table: the FBUS_INFO_NOISE_RESIDENT enumerator in the header and its
mirror in fbus_ekf.capi, the unchanged ABI version, and the two kernel families of build.py (fp32 only) with the unit count
that follows from the FAMILIES table."""
import importlib.util
import os
import re

from fbus_ekf import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_module():
    spec = importlib.util.spec_from_file_location("fbus_build_table", os.path.join(ROOT, "fbus-ekf_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_enumerator_is_in_the_header_and_mirrored():
    hdr = open(capi._HEADER).read()
    m = re.search(r"FBUS_INFO_NOISE_RESIDENT\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == 11
    assert capi.INFO_NOISE_RESIDENT == 11
    # the enumerators in front of it keep their values
    assert capi.INFO_MEAS_SPLIT == 10 and capi.INFO_TEAM_FRAMES == 9 and capi.INFO_SIMDS == 0
    assert re.search(r"FBUS_INFO_MEAS_SPLIT\s*=\s*10\b", hdr)


def test_abi_version_is_unchanged():
    lib = capi.load_library()
    assert capi.ABI_VERSION == 8 and lib.fbus_ekf_abi_version() == 8
    assert re.search(r"#define\s+FBUS_ABI_VERSION\s+8\b", open(capi._HEADER).read())


def test_families_hold_the_tabled_windows_fp32_only():
    b = _build_module()
    by_code = {code: (name, like, f64) for name, (code, like, f64) in b.FAMILIES.items()}
    assert len(by_code) == len(b.FAMILIES)                          # no family number twice
    assert by_code[19][1:] == ("frames", False)                      # family 10's window with (TrajOut, NoiseIn)
    assert by_code[20][1:] == ("fmeas", False)                       # family 11's
    assert by_code[10][1:] == ("frames", False) and by_code[11][1:] == ("fmeas", False)
    tu = open(os.path.join(ROOT, "fbus-ekf_amd", "csrc", "kernels_tu.hip")).read()
    assert re.search(r"FBUS_TU_FAMILY == 19 \|\| FBUS_TU_FAMILY == 20\s*\n#define FBUS_TU_PACK , TrajOut<FBUS_TU_T>, NoiseIn\b", tu)


def test_unit_count_is_the_expansion_of_the_table():
    b = _build_module()
    f32 = len(b.FAMILIES)
    f64 = sum(1 for _, _, on in b.FAMILIES.values() if on)
    units = b.units()
    # every row for fp32, the rows marked so for fp64, each for N = 18 and N = 15; the host unit; the kernels built once
    assert len(units) == 2 * (f32 + f64) + 1 + 1 == 82
    names = [u[0] for u in units]
    assert len(set(names)) == len(names)
    assert "main" in names and "common" in names
    fam19 = [n for n, (code, _, _) in b.FAMILIES.items() if code == 19][0]
    fam20 = [n for n, (code, _, _) in b.FAMILIES.items() if code == 20][0]
    for fam, code in ((fam19, 19), (fam20, 20)):
        for n in (18, 15):
            assert f"f32_{n}_{fam}" in names and f"f64_{n}_{fam}" not in names
            defs = [u[2] for u in units if u[0] == f"f32_{n}_{fam}"][0]
            assert f"-DFBUS_TU_FAMILY={code}" in defs and "-DFBUS_TU_T=float" in defs and f"-DFBUS_TU_N={n}" in defs
    # the README states the count
    assert "82 units" in open(os.path.join(ROOT, "README.md")).read()


def test_the_host_unit_holds_no_kernel_and_the_small_families_take_the_base_flags():
    main = open(os.path.join(ROOT, "fbus-ekf_amd", "csrc", "fbus_ekf.hip")).read()
    assert "__global__" not in main and "hipLaunchKernelGGL" not in main
    included = re.findall(r'#include "(ekf_\w+\.hpp)"', main)
    assert included and set(included) <= {"ekf_launch.hpp", "ekf_route.hpp"}
    b = _build_module()
    small = {"state", "group", "sensor", "screen", "report"}
    assert small <= set(b.FAMILIES) and all(b.FAMILIES[f][2] for f in small)        # fp64 records too
    t_of = {"f32": "float", "f64": "double"}
    seen = 0
    for name, src, defs in b.units():
        tn, _, rest = name.partition("_")
        n, _, fam = rest.partition("_")
        if fam in small:
            assert defs == [f"-DFBUS_TU_T={t_of[tn]}", f"-DFBUS_TU_N={n}", f"-DFBUS_TU_FAMILY={b.FAMILIES[fam][0]}"], name
            assert os.path.basename(src) == "small_tu.hip"
            seen += 1
    assert seen == 4 * len(small)
