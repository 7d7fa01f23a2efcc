"""Pure Python reference of the CIGAR stage (dpx_batch_cigars_begin / _end).  TEST INFRASTRUCTURE ONLY -- never imported by the product.

A column of the three traceback lines is classified by its relation and query-line characters, as include/dpx_align.h states it:
    relation '*'                    '='  consumes both
    relation '|'                    'X'  consumes both
    relation ' ', query line '_'    'D'  consumes the reference only
    relation ' ', anything else     'I'  consumes the query only
The reference line takes no part."""

OP_M, OP_I, OP_D, OP_EQ, OP_X = 0, 1, 2, 7, 8
FLAG_EXTENDED, FLAG_M = 0, 1
LETTERS = {OP_M: "M", OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}


def _bytes(x):
    return x.encode("latin-1") if isinstance(x, str) else bytes(x)


def classify(rel: int, qry: int) -> int:
    if rel == ord("*"):
        return OP_EQ
    if rel == ord("|"):
        return OP_X
    return OP_D if qry == ord("_") else OP_I


def records_and_ops(lines, end_row: int, end_col: int, flags: int = FLAG_EXTENDED):
    """(record, ops) of one pair: `lines` = (reference, relation, query) line, str or bytes; the record is a dict with every field of
    struct dpx_alignment but opsOffset, the ops are a list of (length << 4) | code in path order."""
    ref, rel, qry = (_bytes(x) for x in lines)
    assert len(ref) == len(rel) == len(qry)
    count = {OP_EQ: 0, OP_X: 0, OP_D: 0, OP_I: 0}
    runs = []  # [code, length]
    for r, q in zip(rel, qry):
        cls = classify(r, q)
        count[cls] += 1
        code = OP_M if (flags & FLAG_M) and cls in (OP_EQ, OP_X) else cls
        if runs and runs[-1][0] == code:
            runs[-1][1] += 1
        else:
            runs.append([code, 1])
    on_ref = count[OP_EQ] + count[OP_X] + count[OP_D]
    on_qry = count[OP_EQ] + count[OP_X] + count[OP_I]
    record = {"numOps": len(runs), "refStart": end_col - on_ref, "refEnd": end_col, "qryStart": end_row - on_qry, "qryEnd": end_row,
              "matches": count[OP_EQ], "mismatches": count[OP_X], "insertions": count[OP_I], "deletions": count[OP_D], "reserved": 0}
    return record, [(length << 4) | code for code, length in runs]


def text(ops) -> str:
    return "".join(f"{int(op) >> 4}{LETTERS[int(op) & 15]}" for op in ops) or "*"


def batch(lines_per_pair, end_rows, end_cols, flags: int = FLAG_EXTENDED):
    """(records, ops) of a batch: the records carry opsOffset (exclusive prefix of numOps), the ops are one flat list"""
    records, flat = [], []
    for lines, er, ec in zip(lines_per_pair, end_rows, end_cols):
        rec, ops = records_and_ops(lines, int(er), int(ec), flags)
        rec["opsOffset"] = len(flat)
        records.append(rec)
        flat.extend(ops)
    return records, flat
