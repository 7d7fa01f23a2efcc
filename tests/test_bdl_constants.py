"""DPX_KEEP_LOCAL_BAND_DIRECTIONS on the CPU: the header defines the bit with one comment block that states the contract, the binding
holds the same value and it collides with no other flag, the ABI version stays, and dpx_main's usage text names the combination and
passes the flag.  No GPU is touched."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCPP = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "hostcpp")


def test_header_and_binding_agree_on_the_flag():
    import dpx_gpu_genomics_project_amd as dpx

    header = open(os.path.join(ROOT, "include", "dpx_align.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"#define\s+DPX_KEEP_LOCAL_BAND_DIRECTIONS\s+(0x[0-9a-fA-F]+)u", flat)
    assert m and int(m.group(1), 16) == 0x40 == dpx.KEEP_LOCAL_BAND_DIRECTIONS == dpx.capi.KEEP_LOCAL_BAND_DIRECTIONS
    others = dpx.SCORE_ONLY | dpx.TIME_FILLS | dpx.TUNE_PLACEMENT | dpx.KEEP_DIRECTIONS | dpx.KEEP_BAND_DIRECTIONS | dpx.TWO_PIECE_GAPS
    assert dpx.KEEP_LOCAL_BAND_DIRECTIONS & others == 0
    assert "#define DPX_ABI_VERSION 3" in header  # no bump
    start = header.index("#define DPX_KEEP_LOCAL_BAND_DIRECTIONS")
    block = header[start:header.index("*/", start)]
    for said in ("BSW / BASW", "k_bdl_fill", "k_bdl_traceback", "dpx_banddir.h", "2^28", "DPX_ERR_RANGE", "DPX_ERR_INVALID", "DPX_ERR_UNSUPPORTED",
                 "DPX_ERR_NO_MATRIX", "t == 0", "GAP_OPEN / GAP_EXTEND", "DPX_TB_WALK has no effect", "Every setter refuses",
                 "ignores the", "k_banded_fill", "k_basw_fill"):
        assert said in block, said
    assert "BASW are follow-ups" not in header and "BSW / BASW directions are not implemented" not in header


def test_dpx_main_usage_names_the_combination_and_the_source_passes_the_flag():
    subprocess.run(["make", "-s", "-C", HOSTCPP, "dpx_main"], check=True)
    r = subprocess.run([os.path.join(HOSTCPP, "dpx_main")], capture_output=True, text=True)
    assert r.returncode != 0 and r.stderr.startswith("usage: dpx_main") and r.stdout == ""
    assert "-algo BSW|BASW -directions" in r.stderr
    source = open(os.path.join(HOSTCPP, "dpx_main.cpp")).read()
    assert "DPX_KEEP_LOCAL_BAND_DIRECTIONS" in source
