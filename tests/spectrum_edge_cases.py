"""The tables behind tests/test_gpu_spectrum_edges.py: the spectrum family (sdrhip_spectrum_run_device, sdrhip_spectrum_reduce_run_device:
kernels_spectrum.hip, fft.cpp) on the shapes at which its host loops take a second turn, on offset bases, on directed inputs with a
closed form, and on the float32 value classes.  No pytest and no device in here: tests/test_spectrum_edge_cases.py shows on the CPU
what every case reaches.

A. Slices, chunks and grids.  fft.cpp bounds its scratch at SCRATCH = 64 MiB and the kernels cap their grids; the functions below restate
the host's integer arithmetic (run_chunks, reduce_batches, layer_slices) and every case carries the count of hipFFT transforms or of
layered launches it predicts from them, which the GPU tests read back from sdrhip_debug_spectrum_hipfft_batches and
sdrhip_debug_spectrum_reduce_layer_launches: a change of the scratch size cannot silently turn a case into a one-slice run.

B. Directed inputs: a unit impulse under a Hamming window (every bin is scale * w[j]) and a tone on an exact bin (the peak by a plain
n-term sum), neither through numpy's FFT.

C. float32 value classes of cf32 input: subnormal samples whose outputs are float32 subnormals, samples up to FLT_MAX, outputs past
FLT_MAX, tiny and huge samples in one row.

D. Non-finite cf32 input: where the poisoned sample stands and which rows hold it."""
import dataclasses

import numpy as np

import spectrum_model as M

SCRATCH = 64 << 20                  # SPECTRUM_SCRATCH_BYTES
CHUNK = 32                          # SPECTRUM_REDUCE_CHUNK
GRID_Y_CAP = 4096                   # spectrum_prepare, spectrum_accumulate: gridDim.y
FUSED_GRID = 2048                   # spectrum_fused, spectrum_fused_reduce: tiles resident in one launch
FUSED_SIZES = (64, 128, 256, 512, 1024, 2048, 4096, 8192)
IQ_I16 = 2
FLT_MAX = float(np.finfo(np.float32).max)
FLT_TINY = 2.0 ** -149              # the smallest float32 subnormal


def ceil_div(a, b):
    return (a + b - 1) // b


def rows_per_tile(n):
    """Rows one workgroup of the one-kernel route transforms at a time."""
    return 1 if n >= 2048 else 2048 // n


def samples_for(n, hop, rows):
    return (rows - 1) * hop + n


def u8_iq(seed, n_samples):
    return np.random.default_rng(seed).integers(0, 256, 2 * n_samples, dtype=np.uint8)


# ---- A. the host's arithmetic ---------------------------------------------------------------------------------------------------------
def run_chunks(n, rows):
    """spectrum_run_hipfft: the row counts of the hipFFT transforms of one run_device call."""
    chunk = min(max(SCRATCH // (16 * n), 1), rows)
    return [min(chunk, rows - r0) for r0 in range(0, rows, chunk)]


def reduce_batches(n, rows_out, group):
    """spectrum_reduce_hipfft: [(slice's first output row, first input row of the batch within the slice, input rows)]."""
    rows_slice = min(max(SCRATCH // 2 // (16 * n), 1), rows_out)
    batch = min(max(SCRATCH // 2 // (16 * n), 1), rows_slice * group)
    out = []
    for r0 in range(0, rows_out, rows_slice):
        in_rows = min(rows_slice, rows_out - r0) * group
        out += [(r0, b0, min(batch, in_rows - b0)) for b0 in range(0, in_rows, batch)]
    return out


def layer_slices(n, rows_out, group):
    """spectrum_reduce_fused, groups of more than one chunk: [(first output row, output rows, first chunk, end chunk)] per launch."""
    rpt, nchunks, row_bytes = rows_per_tile(n), ceil_div(group, CHUNK), 8 * n
    rows_slice = SCRATCH // 16 // row_bytes
    if rows_slice > rpt:
        rows_slice -= rows_slice % rpt
    rows_slice = min(max(rows_slice, 1), rows_out)
    layers_slice = min(max(SCRATCH // (rows_slice * row_bytes) - 1, 1), nchunks)
    return [(r0, min(rows_slice, rows_out - r0), c0, min(c0 + layers_slice, nchunks))
            for r0 in range(0, rows_out, rows_slice) for c0 in range(0, nchunks, layers_slice)]


@dataclasses.dataclass(frozen=True)
class RunHipfft:
    """run_device on the hipFFT route; `then_rows`: a second run on the SAME object, whose last chunk needs another plan."""
    n: int
    rows: int
    hop: int
    what: str
    then_rows: int = 0

    @property
    def batches(self):
        return len(run_chunks(self.n, self.rows))

    @property
    def then_batches(self):
        return len(run_chunks(self.n, self.then_rows)) if self.then_rows else 0


RUN_HIPFFT = [
    RunHipfft(16384, 520, 7, "chunks 256 + 256 + 8, then 256 + 44: the plan for 8 rows is replaced by the plan for 44", then_rows=300),
    RunHipfft(1000, 4200, 3, "chunks 4194 + 6: spectrum_prepare's gridDim.y capped at 4096"),
    RunHipfft(1 << 22, 3, 5, "one row fills the scratch: chunks of one row"),
]


@dataclasses.dataclass(frozen=True)
class ReduceHipfft:
    n: int
    rows_out: int
    group: int
    hop: int
    edge: str                   # what the batch edges are named for: "mid-chunk", "fold", "group start", "row slices", "grid"
    what: str
    force: bool = False         # a one-kernel size sent to the hipFFT route
    dirty_group: int = 0        # a run with this group first, on the same object: it leaves state where this case must not load any

    @property
    def batches(self):
        return len(reduce_batches(self.n, self.rows_out, self.group))

    @property
    def edges(self):
        """(position j within its group, slice's first output row) of the first input row of every batch but a slice's first"""
        return [(b0 % self.group, r0) for r0, b0, _ in reduce_batches(self.n, self.rows_out, self.group) if b0 != 0]


def stored_rows(n, rows_out, group):
    """Output rows (of the one slice) whose state a batch of this shape leaves in the scratch: the groups a batch ends inside."""
    return sorted({(b0 + nrows) // group for r0, b0, nrows in reduce_batches(n, rows_out, group) if r0 == 0 and (b0 + nrows) % group})


REDUCE_HIPFFT = [
    ReduceHipfft(16384, 3, 100, 5, "mid-chunk", "batch edges at input rows 128 and 256: j = 28 and 56, state carried mid-chunk"),
    ReduceHipfft(16384, 2, 160, 5, "fold", "batch edge at j = 128 of group 0: the carried chunk is folded on a batch's first row"),
    ReduceHipfft(16384, 5, 64, 3, "group start", "both batch edges on a group's first row: no state may be loaded",
                 dirty_group=60),
    ReduceHipfft(16384, 130, 3, 1, "row slices", "two slices of output rows (128 + 2): 3 + 1 batches"),
    ReduceHipfft(64, 5000, 2, 3, "grid", "5000 output rows in one spectrum_accumulate launch, 10000 input rows in one spectrum_prepare", force=True),
]
ALL_PAIRS_CASE = REDUCE_HIPFFT[0]           # the one case run on all six reduce x unit pairs


@dataclasses.dataclass(frozen=True)
class RunFused:
    n: int
    rows: int
    hop: int
    what: str

    @property
    def tiles(self):
        return ceil_div(self.rows, rows_per_tile(self.n))

    @property
    def second_turn_row(self):
        """The first row of a workgroup's second turn through the tile loop."""
        return FUSED_GRID * rows_per_tile(self.n)


RUN_FUSED = [
    RunFused(2048, 2050, 16, "2050 tiles of one row on a grid of 2048"),
    RunFused(64, 65570, 1, "2050 tiles of 32 rows, the last one partial (2 rows)"),
]


@dataclasses.dataclass(frozen=True)
class ReduceLayers:
    n: int
    rows_out: int
    group: int
    hop: int
    model_rows: tuple           # output rows held against the model: the last of slice 0, the first and the last of slice 1
    what: str

    @property
    def launches(self):
        return len(layer_slices(self.n, self.rows_out, self.group))


REDUCE_LAYERS = ReduceLayers(2048, 300, 500, 16, (255, 256, 299), "two slices of output rows (256 + 44) x two slices of chunks (15 + 1)")


# ---- every size and format of the one-kernel route ------------------------------------------------------------------------------------
def size_case(n):
    """(rows, hop): one row more than a tile (a partial last tile), an odd hop below n."""
    return rows_per_tile(n) + 1, n // 2 - 1


def format_input(fmt, seed, n_samples):
    """(what the device reads, the float32 cf32 buffer the model reads) for u8 / cf32 / int16."""
    rng = np.random.default_rng(seed)
    if fmt == M.IQ_U8:
        iq = rng.integers(0, 256, 2 * n_samples, dtype=np.uint8)
        return iq, ((iq.astype(np.float64) - 128.0) / 128.0).astype(np.float32)         # exact in float32
    if fmt == M.IQ_CF32:
        iq = rng.standard_normal(2 * n_samples).astype(np.float32)
        return iq, iq
    iq = rng.integers(-32768, 32768, 2 * n_samples, dtype=np.int16)
    return iq, (iq.astype(np.float64) * 2.0 ** -11).astype(np.float32)                   # s * 2^-11: exact in float32


# ---- B. directed inputs ---------------------------------------------------------------------------------------------------------------
DIRECTED_SIZES = (64, 512, 4096, 8192, 1000)        # 1000: the hipFFT route


def impulse_positions(n):
    return (0, 1, n // 4, n // 2, n - 1)


def tone_bins(n):
    return (0, 1, n // 4, n // 2 - 1, n // 2, n - 1)


def impulse(n, j):
    iq = np.zeros(2 * n, np.float32)
    iq[2 * j] = 1.0
    return iq


def tone(n, k):
    """exp(2 pi i k j / n) rounded to float32, and the exact |sum_j x[j] exp(-2 pi i k j / n)| of the rounded samples (a plain sum)."""
    ph = 2.0 * np.pi * ((k * np.arange(n)) % n) / n
    iq = np.empty(2 * n, np.float32)
    iq[0::2], iq[1::2] = np.cos(ph), np.sin(ph)
    x = iq[0::2].astype(np.float64) + 1j * iq[1::2].astype(np.float64)
    return iq, float(abs(np.sum(x * np.exp(-1j * ph))))


# ---- C. float32 value classes of cf32 input -------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class ValueClass:
    name: str
    n: int
    rows: int
    scale: float
    make: object                # seed -> float32 interleaved samples, rows * n of them (hop = n)
    overflows: bool = False

    def iq(self):
        return self.make(np.random.default_rng(len(self.name) + self.n), 2 * self.rows * self.n)


def _subnormal(rng, count):
    return (rng.integers(-(1 << 22), 1 << 22, count).astype(np.float64) * FLT_TINY).astype(np.float32)       # |x| < 2^-127: exact


def _huge(rng, count):
    x = rng.uniform(-1.0, 1.0, count) * FLT_MAX
    x[:4] = (FLT_MAX, -FLT_MAX, FLT_MAX, FLT_MAX)
    return x.astype(np.float32)


def _mixed(rng, count):
    x = _huge(rng, count).astype(np.float64) * 2.0 ** -20
    tiny = _subnormal(rng, count)
    pick = rng.integers(0, 2, count).astype(bool)
    return np.where(pick, x, tiny).astype(np.float32)


def value_classes(n):
    """hop = n, no window.  |X| <= n sqrt(2) max|x|: scale 1 / (2 n) keeps FLT_MAX-scale input below FLT_MAX; the overflow case's scale
    puts the middle of the bins' distribution (|X| ~ FLT_MAX sqrt(2 n / 3)) at FLT_MAX."""
    rows = 3
    return [ValueClass("subnormal in, subnormal out", n, rows, 1.0 / n, _subnormal),
            ValueClass("up to FLT_MAX, below it out", n, rows, 1.0 / (2 * n), _huge),
            ValueClass("past FLT_MAX out", n, rows, 1.25 / np.sqrt(2.0 * n / 3.0), _huge, overflows=True),
            ValueClass("tiny and huge in one row", n, rows, 1.0 / n, _mixed)]


def reference(iq, n, scale, hop, rows, kind=M.WINDOW_NONE, shift=False):
    """cf32 input -> rows x n float64 before the final rounding (which may overflow: that is a case here, not a warning)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return M.spectrum(iq, n, M.IQ_CF32, kind, None, shift, scale, hop, rows)[0]


VALUE_CLASS_SIZES = (256, 1000)     # the one-kernel route, the hipFFT route
F32_OVERFLOW = FLT_MAX + 2.0 ** 103       # float32(v) is +Inf from here on (half a unit past FLT_MAX, the tie going to the even Inf)


def close_bound(ref64):
    """The operator's contract, every bin within 1e-11 of the row's largest bin plus one float32 unit in the last place of its own
    value: 2^-23 |ref| at normal magnitudes, as tests/test_gpu_spectrum.py writes it, and the subnormal spacing 2^-149 below."""
    return 1e-11 * np.max(np.abs(ref64), axis=-1, keepdims=True) + np.maximum(2.0 ** -23 * np.abs(ref64), FLT_TINY)


def overflow_split(ref64):
    """-> (must be +Inf, must be finite and close, left out): a bin whose reference lies within the tolerance of the overflow point may
    round either way."""
    near = np.abs(ref64 - F32_OVERFLOW) <= close_bound(ref64)
    return (ref64 >= F32_OVERFLOW) & ~near, (ref64 < F32_OVERFLOW) & ~near, near


# ---- D. non-finite cf32 input ---------------------------------------------------------------------------------------------------------
NONFINITE_SIZES = ((256, 1), (1000, 0))           # (n, route): the one-kernel route, the hipFFT route
NONFINITE_GROUPS = ((3, 4), (70, 3))              # (group, rows_out)
# (name, value, imaginary part?, at j = 0 of a row?)
POISONS = (("NaN re", np.nan, False, False), ("+Inf re", np.inf, False, False), ("-Inf im", -np.inf, True, False),
           ("NaN at j = 0 under w = 0", np.nan, False, True))


def poison_place(n, group, at_j0):
    """hop = n / 2.  -> (sample index, the two input rows that hold it): the last row of output row 0 and the first of output row 1,
    so two output rows are poisoned and the later ones are not."""
    hop, k = n // 2, group
    return k * hop + (0 if at_j0 else 17), (k - 1, k)


def rows_holding(n, hop, rows, p):
    return [r for r in range(rows) if r * hop <= p < r * hop + n]


def poisoned(iq, p, value, imaginary):
    out = iq.copy()
    out[2 * p + (1 if imaginary else 0)] = value
    return out
