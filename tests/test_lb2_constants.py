"""DPX_LOCAL_TWO_PIECE_GAPS on the CPU: the header defines the bit with one comment block that states the contract, the binding holds
the same value and it collides with no other flag, the ABI version and the symbol list stay, the new kernel unit is one of the library's,
and dpx_main's usage text names -localopen2 / -localextend2 and refuses their misuse before any device is touched.  No GPU is touched."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCPP = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "hostcpp")
CSRC = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "csrc")


def test_header_and_binding_agree_on_the_flag():
    import dpx_gpu_genomics_project_amd as dpx

    header = open(os.path.join(ROOT, "include", "dpx_align.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"#define\s+DPX_LOCAL_TWO_PIECE_GAPS\s+(0x[0-9a-fA-F]+)u", flat)
    assert m and int(m.group(1), 16) == 0x80 == dpx.LOCAL_TWO_PIECE_GAPS == dpx.capi.LOCAL_TWO_PIECE_GAPS
    assert "LOCAL_TWO_PIECE_GAPS" in dpx.__all__
    others = (dpx.SCORE_ONLY | dpx.TIME_FILLS | dpx.TUNE_PLACEMENT | dpx.KEEP_DIRECTIONS | dpx.KEEP_BAND_DIRECTIONS | dpx.TWO_PIECE_GAPS |
              dpx.KEEP_LOCAL_BAND_DIRECTIONS)
    assert dpx.LOCAL_TWO_PIECE_GAPS & others == 0
    assert "#define DPX_ABI_VERSION 3" in header  # no bump, and no new symbol
    assert "dpx_batch_set_second_gap" in dpx.capi.ABI_SYMBOLS and not any("lb2" in s or "local_two" in s for s in dpx.capi.ABI_SYMBOLS)
    end = header.index("#define DPX_LOCAL_TWO_PIECE_GAPS")
    block = header[header.rindex("/* ----", 0, end):end]
    for said in ("DPX_KEEP_LOCAL_BAND_DIRECTIONS", "DPX_ALGO_BASW", "dpx_batch_set_second_gap", "without a two-piece flag", "no ABI bump",
                 "H = 0 and D1 = D2 = I1 = I2", "GAP_OPEN wins a tie", "D1, D2, I1, I2", "H = max(0, winner)", "NONE where H == 0",
                 "first maximum in row-major order", "Five states", "An edge cell always opens", "six selectors", "DPX_MAT_H_PIECE",
                 "k_lb2_fill", "k_lb2_traceback", "matrix=banddir8 gap2=<o2>,<e2>", "B <= 256", "DPX_ERR_UNSUPPORTED", "DPX_ERR_INVALID",
                 "2^28", "dpx_batch_set_local_direction_table is admitted", "160 KiB", "byte-identical", "k_bdl_fill", "BSW included"):
        assert said in block, said


def test_the_unit_is_one_of_the_librarys():
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "dpx_lb2_kernels.hip" in makefile and os.path.exists(os.path.join(CSRC, "dpx_lb2_kernels.hip"))


def test_dpx_main_usage_names_the_local_second_piece_and_refuses_misuse(tmp_path):
    subprocess.run(["make", "-s", "-C", HOSTCPP, "dpx_main"], check=True)
    main = os.path.join(HOSTCPP, "dpx_main")
    r = subprocess.run([main], capture_output=True, text=True)
    assert r.returncode != 0 and r.stderr.startswith("usage: dpx_main") and r.stdout == ""
    assert "[-localopen2 <O2> -localextend2 <E2>]" in r.stderr and "only with -directions and -algo BASW" in r.stderr
    # (-open2 / -extend2 keep their text)
    assert "[-open2 <O2> -extend2 <E2>]" in r.stderr and "only with -directions and -algo BANW|BAXT" in r.stderr
    pairs = tmp_path / "none.txt"  # never opened: every misuse is refused first
    both = ["-localopen2", "-24", "-localextend2", "-1"]
    for args in (["-algo", "BASW", "-directions", "-localopen2", "-24"], ["-algo", "BASW", "-directions", "-localextend2", "-1"],  # one without the other
                 ["-algo", "BASW"] + both,                                                # without -directions
                 ["-algo", "BSW", "-directions"] + both,                                  # BSW has no second piece
                 ["-algo", "ASW", "-directions"] + both, ["-algo", "BANW", "-directions"] + both, ["-algo", "BAXT", "-directions"] + both,
                 ["-algo", "LSW", "-directions"] + both,
                 ["-algo", "BASW", "-directions", "-open2", "-24", "-extend2", "-1"] + both,  # not with the other pair of flags
                 ["-algo", "BASW", "-directions", "-open2", "-24", "-extend2", "-1"],         # which stay BANW's / BAXT's
                 ["-algo", "BASW", "-scores"] + both, ["-algo", "BASW", "-scores", "-directions"] + both):
        r = subprocess.run([main, "-pairs", str(pairs)] + args, capture_output=True, text=True)
        assert r.returncode != 0 and r.stderr.startswith("usage: dpx_main") and r.stdout == "", args  # (before any device is touched)
    source = open(os.path.join(HOSTCPP, "dpx_main.cpp")).read()
    assert "DPX_LOCAL_TWO_PIECE_GAPS" in source and "dpx_batch_set_second_gap" in source
