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
    assert len(units) == 1 + 2 * (f32 + f64) == 61
    names = [u[0] for u in units]
    assert len(set(names)) == len(names)
    fam19 = [n for n, (code, _, _) in b.FAMILIES.items() if code == 19][0]
    fam20 = [n for n, (code, _, _) in b.FAMILIES.items() if code == 20][0]
    for fam, code in ((fam19, 19), (fam20, 20)):
        for n in (18, 15):
            assert f"f32_{n}_{fam}" in names and f"f64_{n}_{fam}" not in names
            defs = [u[2] for u in units if u[0] == f"f32_{n}_{fam}"][0]
            assert f"-DFBUS_TU_FAMILY={code}" in defs and "-DFBUS_TU_T=float" in defs and f"-DFBUS_TU_N={n}" in defs
    # the README states the count
    assert "61 units" in open(os.path.join(ROOT, "README.md")).read()
