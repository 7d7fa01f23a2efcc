"""Pure Python reference of the difference strings (dpx_batch_diffs_begin / _end).  TEST INFRASTRUCTURE ONLY -- never imported by the
product.

Columns of the three traceback lines are classified as tests/cigar_ref.py classifies them ('*' -> '=', '|' -> 'X', otherwise a gap:
query byte '_' -> 'D', anything else -> 'I'); include/dpx_align.h states both formats:

    MD  (samtools calmd)   n = '=' columns since the last X or the last start of a D run; X: decimal(n) ref; first D of a run:
                           decimal(n) '^' ref; further D: ref; I: nothing (but it ends a D run); at the end: decimal(n)
    cs  (minimap2, short)  '=' run of L: ':' decimal(L); X: '*' lc(ref) lc(qry); I run: '+' lc(qry)...; D run: '-' lc(ref)...

Strings are bytes: the lines may hold any byte."""
import re


def _bytes(x):
    return x.encode("latin-1") if isinstance(x, str) else bytes(x)


def classes(lines) -> str:
    """the class string of a pair's lines, one of = X D I per column"""
    _, rel, qry = (_bytes(x) for x in lines)
    assert len(rel) == len(qry)
    return "".join("=" if r == 0x2A else "X" if r == 0x7C else "D" if q == 0x5F else "I" for r, q in zip(rel, qry))


def lc(b: int) -> int:
    return b + 32 if 0x41 <= b <= 0x5A else b


def md(lines) -> bytes:
    ref = _bytes(lines[0])
    out, n, prev = bytearray(), 0, None
    for c, cls in enumerate(classes(lines)):
        if cls == "=":
            n += 1
        elif cls == "X":
            out += b"%d" % n
            out.append(ref[c])
            n = 0
        elif cls == "D":
            if prev != "D":
                out += b"%d^" % n
                n = 0
            out.append(ref[c])
        prev = cls
    out += b"%d" % n
    return bytes(out)


def cs(lines) -> bytes:
    ref, qry = _bytes(lines[0]), _bytes(lines[2])
    out = bytearray()
    for m in re.finditer(r"=+|X|I+|D+", classes(lines)):
        cls, lo, hi = m.group(0)[0], m.start(), m.end()
        if cls == "=":
            out += b":%d" % (hi - lo)
        elif cls == "X":
            out += bytes((0x2A, lc(ref[lo]), lc(qry[lo])))
        elif cls == "I":
            out += b"+" + bytes(lc(b) for b in qry[lo:hi])
        else:
            out += b"-" + bytes(lc(b) for b in ref[lo:hi])
    return bytes(out)


KINDS = {1: md, 2: cs}  # DPX_DIFF_MD, DPX_DIFF_CS


def lines_of(class_string: str, ref_bases: bytes = b"ACGT", qry_bases: bytes = b"ACGT"):
    """three lines with the given classes: the engine's conventions ('_' in the gapped line, ' ' in the relation line of a gap), bases
    cycling through `ref_bases` / `qry_bases`, a mismatch's query base the next one of the cycle"""
    ref, rel, qry = bytearray(), bytearray(), bytearray()
    for c, cls in enumerate(class_string):
        a = ref_bases[c % len(ref_bases)]
        if cls == "=":
            ref.append(a); rel.append(0x2A); qry.append(a)
        elif cls == "X":
            ref.append(a); rel.append(0x7C); qry.append(qry_bases[(c + 1) % len(qry_bases)])
        elif cls == "D":
            ref.append(a); rel.append(0x20); qry.append(0x5F)
        else:
            ref.append(0x5F); rel.append(0x20); qry.append(qry_bases[c % len(qry_bases)])
    return bytes(ref), bytes(rel), bytes(qry)


def parse_md(text: bytes):
    """(matches, mismatches, deletions) of an MD string whose reference bytes are letters"""
    matches = mismatches = deletions = 0
    for tok in re.finditer(rb"(\d+)|\^([A-Za-z]+)|([A-Za-z])", text):
        if tok.group(1) is not None:
            matches += int(tok.group(1))
        elif tok.group(2) is not None:
            deletions += len(tok.group(2))
        else:
            mismatches += 1
    return matches, mismatches, deletions


def parse_cs(text: bytes) -> str:
    """the class string a short cs string (lower-case letters) stands for"""
    out, seen = [], 0
    for tok in re.finditer(rb":(\d+)|\*([a-z_])([a-z_])|\+([a-z_]+)|-([a-z_]+)", text):
        seen += len(tok.group(0))
        if tok.group(1) is not None:
            out.append("=" * int(tok.group(1)))
        elif tok.group(2) is not None:
            out.append("X")
        elif tok.group(4) is not None:
            out.append("I" * len(tok.group(4)))
        else:
            out.append("D" * len(tok.group(5)))
    assert seen == len(text), text  # every byte belongs to a token
    return "".join(out)
