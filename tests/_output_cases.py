"""Shared cases of the Output-field tests (``test_batch_outputs.py`` on the CPU,
``test_gpu_outputs.py`` on the GPU): a document editor, raw-result generators and a direct
per-row evaluation of the output kernel's column program."""

import re

import numpy as np

from flink_jpmml_amd.ops import outputs as K


def bits(a) -> np.ndarray:
    """The bit patterns of an fp32 array (NaN payloads included)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def with_output(text: str, fields: str) -> str:
    """``text`` with its top-level model's ``<Output>`` replaced by (or given) ``fields``, the
    ``<OutputField .../>`` elements. The block goes right behind the first ``MiningSchema``, which
    is the top-level model's in every ``synth`` document."""
    end = text.index("</MiningSchema>") + len("</MiningSchema>")
    rest = re.sub(r"\A\s*<Output>.*?</Output>", "", text[end:], count=1, flags=re.S)  # its own, not a segment's
    return text[:end] + f"\n<Output>{fields}</Output>\n" + rest


def field(name: str, feature: str, data_type: str = "double", optype: str = "continuous", value=None,
          rank=None, inner: str = "") -> str:
    extra = (f' value="{value}"' if value is not None else "") + (f' rank="{rank}"' if rank is not None else "")
    return (f'<OutputField name="{name}" optype="{optype}" dataType="{data_type}" feature="{feature}"{extra}>'
            f'{inner}</OutputField>')


def probability_fields(classes) -> str:
    return "".join(field(f"p_{c}", "probability", value=c) for c in classes)


def raw_results(m: int, C: int, seed: int):
    """``(score, valid, probs or None, affinity)`` of ``m`` rows from ``seed``: class indices (or
    values when ``C == 0``) with invalid rows, NaN scores on valid rows, probabilities with exact
    ties, NaNs, one all-NaN row and one-hot rows."""
    rng = np.random.default_rng(seed)
    valid = (rng.random(m) > 0.15).astype(np.uint8)
    if C:
        score = rng.integers(0, C, m).astype(np.float32)
        # a coarse grid makes exact ties frequent
        probs = (rng.integers(0, 5, (m, C)) / np.float32(4)).astype(np.float32)
        probs[rng.random((m, C)) < 0.05] = np.nan
        probs[rng.integers(0, m)] = np.nan  # an all-NaN row
        hot = rng.integers(0, m, max(1, m // 8))
        probs[hot] = 0.0
        probs[hot, rng.integers(0, C, hot.size)] = 1.0
        if m > 2:
            probs[2] = 0.25  # every class tied
            valid[2] = 1
    else:
        score = rng.standard_normal(m).astype(np.float32)
        probs = None
    score[rng.random(m) < 0.05] = np.nan
    if m > 3:
        score[3] = -1.0  # an index below the table
        valid[3] = 1
    affinity = rng.random(m).astype(np.float32)
    return score, valid, probs, affinity


def program(n_col: int, C: int, k: int, n_labels: int, seed: int):
    """A column program of ``n_col`` columns that uses every op the inputs allow, and its tables
    (two ``n_labels + 1`` encodings with a NaN tail, and two constants)."""
    rng = np.random.default_rng(seed)
    enc = np.concatenate([np.arange(n_labels) * 2.0 + 1.0, [np.nan], rng.permutation(n_labels) + 100.0, [np.nan],
                          [0.0, -7.5]]).astype(np.float32)
    c0 = 2 * (n_labels + 1)
    ops = [(K.OP_VALUE, 0, 0), (K.OP_TABLE, n_labels, 0), (K.OP_TABLE, n_labels, n_labels + 1),
           (K.OP_AFFINITY, 0, 0), (K.OP_CONST, 0, c0), (K.OP_CONST, 0, c0 + 1), (K.OP_NAN, 0, 0)]
    if C:
        ops += [(K.OP_PROB_WINNER, 0, 0)] + [(K.OP_PROB, c, 0) for c in sorted({0, C - 1, C // 2})]
    for r in range(k):
        ops += [(K.OP_TOPK_INDEX, r, 0), (K.OP_TOPK_PROB, r, 0)]
    # the top-k columns first so a small n_col still has them, then the rest round robin
    ops = ops[::-1]
    prog = [ops[j % len(ops)] for j in range(n_col)]
    return np.array([(op, arg, off, 0) for op, arg, off in prog], dtype=np.int32), enc


def top_k_reference(p: np.ndarray, k: int):
    """``np.argsort(-p, kind="stable")`` with the NaNs moved last and dropped."""
    order = [int(c) for c in np.argsort(-p, kind="stable") if not np.isnan(p[c])][:k]
    return order


def evaluate_rows(score, valid, prog, tables, probs, affinity, label_table, k):
    """Each op of the column program evaluated per row in plain Python."""
    m, n_col = len(score), len(prog)
    nan = np.float32(np.nan)
    out = np.full((m, n_col), nan, dtype=np.float32)
    so = np.full(m, nan, dtype=np.float32)
    vo = np.zeros(m, dtype=np.uint8)
    C = probs.shape[1] if probs is not None else 0
    for r in range(m):
        s, ok = score[r], bool(valid[r])
        has_idx = ok and not np.isnan(s)
        top = top_k_reference(probs[r], k) if (C and ok) else []
        for j, (op, arg, off, _) in enumerate(prog):
            x = nan
            if op == K.OP_VALUE:
                x = s if ok else nan
            elif op == K.OP_TABLE:
                idx = int(s) if has_idx and 0 <= s < arg else arg
                x = tables[off + idx]
            elif op == K.OP_PROB:
                x = probs[r, arg] if ok and arg < C else nan
            elif op == K.OP_PROB_WINNER:
                if ok and C:
                    x = probs[r, int(s) if has_idx and 0 <= s < C else 0]
            elif op == K.OP_AFFINITY:
                x = affinity[r] if ok and affinity is not None else nan
            elif op == K.OP_CONST:
                x = tables[off]
            elif op == K.OP_TOPK_INDEX:
                x = np.float32(top[arg]) if arg < len(top) else nan
            elif op == K.OP_TOPK_PROB:
                x = probs[r, top[arg]] if arg < len(top) else nan
            out[r, j] = x
        if label_table is not None:
            L = len(label_table) - 1
            t = label_table[int(s) if has_idx and 0 <= s < L else L]
            if ok and not np.isnan(t):
                so[r], vo[r] = t, 1
        else:
            so[r], vo[r] = s, valid[r] != 0
    return out, so, vo


# the shape grid of the kernel tests: (m, C, n_col, k); R of each (C, n_col) pair decides the 2R + 1 rows
def grid():
    cases = []
    for m in (1, 63, 64, 65, 255, 256, 257):
        cases.append((m, 3, 3, 1))
    for C in (0, 2, 3, 16, 17, 64, 256):
        for n_col, k in ((1, 0), (3, 3), (8, 1), (33, 8), (64, 3)):
            cases.append((2 * K.rows_per_block(C, n_col) + 1, C, n_col, k))
    return cases
