"""Row sets for the row forms of agc and dcBlocker (sdrhip_agc_run_rows / sdrhip_dc_blocker_run_rows): the CPU check
(tests/test_iir_rows_cases.py) and the GPU runs (tests/test_gpu_rows.py) read this one table.

A row set is one call: an operator, n, run_in, (agc) mu and reference -- shared by the rows, as the call shares them -- and per
row a stream of tests/iir_cases.py and a starting state.  Every row is an iir_cases.Case of its own, so the sequential models and
the scheme model of that file say what the row's output, final state and statistics words have to be: a row of a rows call is
the one-row call on that row alone.

mu and reference are per call, so the `range` and `subnormal-parts` streams (mu = 2^-101 and 0.4 * 2^127) cannot stand beside
noise at mu = 0.4: their neighbours are noise rows under the same mu (range: the state then climbs by 2^-11 a sample) and
further streams of their own kind from other seeds and states."""
import dataclasses

import iir_cases as IC


@dataclasses.dataclass(frozen=True)
class RowSet:
    name: str
    op: str                     # "dc" | "agc"
    n: int
    run_in: int
    rows: tuple                 # ((stream key, state tuple), ...)
    reach: str
    mu: float = 0.0
    reference: float = 1.0

    def cases(self):
        return [IC.Case(f"rows/{self.name}/{r}", self.op, strm, self.n, self.run_in, self.reach, state=tuple(state), mu=self.mu,
                        reference=self.reference) for r, (strm, state) in enumerate(self.rows)]


N_AGC, N_DC = 4100, 2051
AGC_QUIET = ("noise", N_AGC, 41, 0.3)
AGC_REPAIRED = ("noise", N_AGC, 45, 0.05)
AGC_WALKED = ("noise", N_AGC, 42, 0.01)
AGC_SILENT = ("noise", N_AGC, 43, 0.0)
DC_FIXED_NOISE = ("fixed_point", N_DC, 1636, 5)

AGC_BRANCHES = RowSet("agc-branches", "agc", N_AGC, 512,
                      ((AGC_QUIET, (1.0,)), (AGC_REPAIRED, (1.0,)), (AGC_WALKED, (1.0,)), (AGC_SILENT, (1.0,))),
                      "no chunk wrong / wrong and repaired by the rounds / left to the walk, in one launch", mu=0.4)
DC_BRANCHES = RowSet("dc-branches", "dc", N_DC, 64,
                     ((IC.UNIFORM, IC.DC_STATE), (IC.CANCEL, IC.DC_STATE), (DC_FIXED_NOISE, (0.75, IC.FIXED_POINT))),
                     "the walk runs to the end / meets the stored trajectory a chunk on / meets it where the noise begins")


def _edges(op, n):
    if op == "dc":
        rows = ((IC.CANCEL, IC.DC_STATE), (IC.UNIFORM, (-1.5, 0.125)), (DC_FIXED_NOISE, (0.75, IC.FIXED_POINT)))
        return RowSet(f"dc-n={n}", "dc", n, 64, rows, "plan edge on three rows at once")
    rows = ((IC.NOISE, (1.0,)), (AGC_REPAIRED, (0.5,)), (AGC_SILENT, (3.0,)))
    return RowSet(f"agc-n={n}", "agc", n, 64, rows, "plan edge on three rows at once", mu=0.4)


EDGE_NS = (127, 128, 129, 0, 1, 7)
EDGES = [_edges(op, n) for op in ("dc", "agc") for n in EDGE_NS]

N_CLASS = 2050
AGC_RANGE = RowSet("agc-range", "agc", N_CLASS, 64,
                   ((("noise", N_AGC, 46, 0.3), (1.0,)), (("agc_range", 8194, 33), (1.0,)), (("agc_range", N_CLASS, 36), (0.75,))),
                   "|x| in 2^60 .. 2^100 beside noise: squares overflow, parts subnormal", mu=IC.RANGE_MU, reference=IC.RANGE_REF)
AGC_SUBNORMAL = RowSet("agc-subnormal-parts", "agc", N_CLASS, 64,
                       ((("agc_subnormal", 8192, 34), (1.0,)), (("agc_subnormal", N_CLASS, 37), (1.25,))),
                       "every corrected part subnormal: frexpf must normalise", mu=IC.SUB_MU, reference=IC.SUB_REF)

SETS = [AGC_BRANCHES, DC_BRANCHES] + EDGES + [AGC_RANGE, AGC_SUBNORMAL]
BY_NAME = {s.name: s for s in SETS}
assert len(BY_NAME) == len(SETS)


def plan_of(lib, rs, rows=None):
    """(chunks per row, C, W) from the library's rows plan hooks: no launch, no device."""
    rows = len(rs.rows) if rows is None else rows
    return lib.dc_rows_plan(rows, rs.n, rs.run_in) if rs.op == "dc" else lib.agc_rows_plan(rows, rs.n, rs.mu, rs.run_in)


def schemes(lib, rs, oracle):
    """Per row, iir_cases.scheme under the plan the rows hook reports."""
    plan = plan_of(lib, rs)
    return [IC.scheme(c, plan, oracle) for c in rs.cases()]
