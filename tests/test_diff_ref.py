"""tests/diff_ref.py against hand-written examples (tests/golden/diff_examples.json), its identities on random lines, and the length
bound include/dpx_align.h derives, exhaustively for every class string of up to 8 columns.  No device, no library."""
import itertools
import json
import os
import random
import re

import cigar_ref
import diff_ref as R

EXAMPLES = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diff_examples.json")))


def _lines(e):
    return e["ref"], e["rel"], e["qry"]


def test_hand_written_examples():
    assert len(EXAMPLES) >= 16
    for e in EXAMPLES:
        assert len(e["ref"]) == len(e["rel"]) == len(e["qry"]), e["what"]
        assert R.md(_lines(e)) == e["md"].encode("latin-1"), e["what"]
        assert R.cs(_lines(e)) == e["cs"].encode("latin-1"), e["what"]


def test_the_examples_cover_what_they_must():
    cls = [R.classes(_lines(e)) for e in EXAMPLES]
    assert "" in cls and all(one in cls for one in "=XDI")  # an empty alignment, a single column of each class
    assert any(c[:1] == "X" and len(c) > 1 for c in cls) and any(c[-1:] == "X" and len(c) > 1 for c in cls)  # a mismatch first / last
    for pattern in ("DX", "XD", "DID", "=I="):
        assert any(pattern in c for c in cls), pattern
    letters = set(range(0x41, 0x5B))
    assert any(set(e["ref"].encode("latin-1")) - letters - {0x5F} for e in EXAMPLES)  # bytes outside A-Z
    # the rows of the interface's table
    table = {e["md"] for e in EXAMPLES}
    assert {"10A5^AC6", "2^AC0T1", "2^AC0^GT1", "0A0C0", "0A0^C0", "4", "0"} <= table
    assert ":3*ta:2+gg:1-tt:1" in {e["cs"] for e in EXAMPLES}


def _random_classes(rng, length):
    weights = rng.choice([(1, 1, 1, 1), (20, 1, 1, 1), (1, 4, 4, 4), (200, 1, 0, 0)])
    return "".join(rng.choices("=XDI", weights=weights, k=length))


def test_identities_on_random_lines():
    rng = random.Random(16)
    for _ in range(400):
        cls = _random_classes(rng, rng.randrange(0, 400))
        lines = R.lines_of(cls)
        assert R.classes(lines) == cls
        rec, ops = cigar_ref.records_and_ops(lines, 0, 0)
        md, cs = R.md(lines), R.cs(lines)
        assert R.parse_md(md) == (rec["matches"], rec["mismatches"], rec["deletions"]), cls
        back = R.parse_cs(cs)
        assert back == cls
        assert (back.count("="), back.count("X"), back.count("I"), back.count("D")) == (rec["matches"], rec["mismatches"], rec["insertions"], rec["deletions"])
        # the runs of cs are the ops of DPX_CIGAR_EXTENDED
        assert cigar_ref.text(ops) == ("".join(f"{len(run)}{run[0]}" for run, _ in re.findall(r"((.)\2*)", back)) or "*")


def test_length_bound_for_every_class_string_up_to_eight_columns():
    """MD <= (5 L + 1) // 2 + 1 and cs <= 3 L, hence both <= 3 * (L + 1) <= 3 * cap: what sizes the device text buffer"""
    worst_md = worst_cs = 0
    for length in range(9):
        for cls in itertools.product("=XDI", repeat=length):
            lines = R.lines_of("".join(cls))
            md, cs = len(R.md(lines)), len(R.cs(lines))
            assert md <= (5 * length + 1) // 2 + 1 and cs <= 3 * length, cls
            assert max(md, cs) <= 3 * (length + 1)
            worst_md, worst_cs = max(worst_md, md - (5 * length + 1) // 2 - 1), max(worst_cs, cs - 3 * length)
    assert worst_md == 0 and worst_cs == 0  # both bounds are met: neither is slack


def test_long_numbers():
    for run in (9, 10, 99, 100, 99999, 100000):
        eq = R.lines_of("=" * run)
        lines = tuple(a + b + a for a, b in zip(eq, (b"C", b"|", b"A")))
        assert R.md(lines) == b"%dC%d" % (run, run) and R.cs(lines) == b":%d*ca:%d" % (run, run)
