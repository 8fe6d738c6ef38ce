"""GPU: the FIR row kernels on the float32 value classes -- signed zeros, subnormals, sums that overflow, Inf and NaN inside a
window, and for one real and one complex family zero taps too (tests/rows_limit_cases.py, section C).

The one-row value-class table (tests/test_gpu_value_classes.py) cannot reach what only the row form has: k_split_rows with U = 1 on
a tile capped at the row's own cycles, and the three *_crossfix_rows kernels, which are restated copies of the generic fix-ups.
Every banked family runs four rows (one unsalted, three cut from salted streams) at a short length (U = 1, capped tile) and a long
one (three tiles of plan_tile's size), each with seams inside the range -- the row fix-up kernels then run on the salted data -- and
without.  Expected values are the restated Pipe on each row's stream, never the device; the banked route is held to them and to the
one-row device call on the row: NaN positions agree, everything else bit for bit (value_classes.assert_same_classes).
tests/test_rows_limit_cases.py shows on the CPU that zeros, subnormals, infinities and NaN all occur in every call's expected
outputs, and per family with seams a NaN Cross output, a finite Cross output over zeros or subnormals, and a non-finite One output
beside a seam."""
import numpy as np
import pytest

import fir_rows_cases as RC
import rows_limit_cases as LC
import value_classes as VC
from test_gpu_fir_rows import desc_of, one_row_calls, run_rows

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("f", LC.CLASS_FAMILIES, ids=[f.name for f in LC.CLASS_FAMILIES])
def test_fir_rows_on_value_classes(hip, oracle, f):
    desc = desc_of(hip, f)
    for case, g in LC.class_cases(hip, f, desc):
        p = g.plan
        seams = RC.seams_inside(f, g.k_begin, g.k_end, g.seam)
        if case.size == "short":
            assert p["per_lane"] == 1 and p["cycles_per_tile"] < p["split_cycles_per_tile"], (case.name, p)
        else:
            assert p["tiles_per_row"] >= 3 and p["per_lane"] == p["split_per_lane"], (case.name, p)
        assert (len(seams) >= (2 if case.size == "short" and f.name in LC.TWO_SEAMS_ONLY else 3)) if case.seam_kind == "three" else not seams
        xs, planted, exp = LC.class_expected(case, g, oracle)
        VC.assert_not_vacuous(np.concatenate(exp), case.name)
        outs, (tiles, fixups, split) = run_rows(hip, case, g, xs, 1, what=case.name)
        print(f"    {case.name}: plan {p}, {len(seams)} seams inside, planted {planted}, tile launches {tiles}, fix-up launches {fixups}")
        assert (tiles, fixups, split) == (1, int(bool(seams)), 0), f"{case.name}: {tiles} tile launches, {fixups} fix-up launches, {split} one-row launches"
        one = one_row_calls(hip, case, g, xs)
        VC.assert_same_classes(np.concatenate(outs), np.concatenate(exp), f"{case.name}: the banked route against the restated Pipe, all rows")
        for r in range(LC.CLASS_ROWS):
            VC.assert_same_classes(outs[r], exp[r], f"{case.name}, row {r}: the banked route against the restated Pipe", max_nan_share=0.5)
            VC.assert_same_classes(outs[r], one[r], f"{case.name}, row {r}: the banked route against the one-row call", max_nan_share=0.5)
