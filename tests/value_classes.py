"""Inputs salted with the float32 value classes the ordinary test signals never contain -- signed zeros, subnormals, tiny and huge
normals, sums that overflow, infinities, NaN -- and the comparison that goes with them.

The FIR kernels contain shortcuts whose exactness depends on the value class (padding taps that are skipped, guarded walks, the
+0 a partial sum starts from, taps pre-scaled by 1/128, the symmetric pre-add): tests/test_oracle_value_classes.py pins the CPU
restatement on these inputs against the reference's own C, tests/test_gpu_value_classes.py pins every kernel family against the
restatement.

NaN: positions are compared, sign and payload are not (x86 generates 0xffc00000, the GPU 0x7fc00000, and which operand's payload
a sum propagates is the compiler's choice).  Everything else -- +-0, subnormals, +-Inf -- is compared bit for bit."""
import numpy as np

from conftest import assert_bit_equal
from ref_answers import RecordedArray, canonical_nan

BLOCK = 8192
FINITE = ("pzero", "nzero", "altzero", "subnormal", "tiny", "large", "sub_in_zero", "lone_nzero", "lone_min")
ISLANDS = ("inf_re", "ninf_im", "nan", "inf_both", "overflow")


def _layout(n, lp, kinds, lengths, every):
    """Segment starts (in samples) of passes over `kinds`: pass 0 starts at sample 1 (an odd start), pass k >= 1 is rotated by k
    kinds and placed so that its first segment straddles the block edge k * every * BLOCK.  Consecutive segments are 2 lp + 1
    samples apart, so no window of lp samples sees two of them."""
    gap = 2 * lp + 1
    table, cursor, k = [], 1, 0
    while True:
        order = kinds[k % len(kinds):] + kinds[:k % len(kinds)]
        if k:
            edge = k * every * BLOCK
            first = lengths[order[0]]
            start = edge - (first // 2 if first > 1 else 1)
            if start < cursor or edge >= n:
                break
            cursor = start
        done = []
        for kind in order:
            if cursor + lengths[kind] + gap > n:
                break
            done.append({"kind": kind, "start": cursor, "len": lengths[kind]})
            cursor += lengths[kind] + gap
        table += done
        if len(done) < len(order):
            assert k, f"the stream of {n} samples is too short for one pass of segments at lp = {lp}"
            break
        k += 1
    return table


def _place_extra(table, extra, lp, lengths, n):
    """The short list (zero run, subnormal run, NaN island) again from each sample position in `extra`."""
    gap = 2 * lp + 1
    for start in extra:
        cursor = int(start)
        for kind in ("pzero", "subnormal", "nan"):
            assert cursor + lengths[kind] <= n, "extra segments run past the stream"
            table.append({"kind": kind, "start": cursor, "len": lengths[kind]})
            cursor += lengths[kind] + gap
    return table


def _bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


def salt(x, width, lp, seed, large=(60, 62), islands=True, every=1, extra=()):
    """A copy of the stream `x` (width floats per sample: 1 real, 2 complex; lp: the longest window of the operator under test, in
    input samples) with the value-class segments planted, and the segment table [{"kind", "start", "len"}] in samples.

    Finite runs of 2 lp samples: pzero, nzero, altzero (+0 / -0 alternating), subnormal (bit patterns 1 .. 0x7fffff, both signs),
    tiny (2^-125 .. 2^-100 on every other sample, ordinary samples between), large (2^large[0] .. 2^large[1], one sign), sub_in_zero
    (three subnormal samples in the middle of zeros: outputs stay subnormal even where one tap is huge, since it mostly meets a zero);
    lone_nzero and lone_min (2^-149) are single samples.  Islands, one sample each with at least 2 lp ordinary samples on either side:
    inf_re (+Inf, real part only), ninf_im (-Inf, imaginary part only), nan (0x7fc00000), inf_both; overflow is a run of lp samples of
    +-3.0e38 with alternating sign.  islands=False leaves the non-finite ones (and overflow) out.  Passes of all segments repeat from
    every `every`-th 8192-sample edge on, so that a segment straddles each of those edges; `extra`: see _place_extra."""
    x = np.array(x, dtype=np.float32, copy=True)
    n = x.size // width
    rng = np.random.default_rng(seed)
    kinds = list(FINITE) + (list(ISLANDS) if islands else [])
    lengths = {k: 2 * lp for k in FINITE[:7]}
    lengths.update(lone_nzero=1, lone_min=1, inf_re=1, ninf_im=1, nan=1, inf_both=1, overflow=lp)
    table = _place_extra(_layout(n, lp, kinds, lengths, every), extra, lp, lengths, n)
    v = x.reshape(n, width)
    for seg in table:
        a, m = seg["start"], seg["len"]
        s = v[a:a + m]
        kind = seg["kind"]
        if kind == "pzero":
            s[:] = 0.0
        elif kind == "nzero":
            s[:] = -0.0
        elif kind == "altzero":
            odd = (np.arange(m)[:, None] + np.arange(width)[None, :]) & 1
            s[:] = np.where(odd, np.float32(-0.0), np.float32(0.0))
        elif kind == "subnormal":
            s[:] = _bits(rng.integers(1, 0x800000, (m, width), dtype=np.uint32) | (rng.integers(0, 2, (m, width), dtype=np.uint32) << 31))
        elif kind == "tiny":
            e = rng.integers(-125, -99, (m, width))
            t = (np.ldexp(1.0, e) * rng.choice([-1.0, 1.0], (m, width))).astype(np.float32)
            s[1::2] = t[1::2]
        elif kind == "large":
            sign = 1.0 if rng.integers(0, 2) else -1.0
            s[:] = (sign * np.ldexp(1.0, rng.integers(large[0], large[1] + 1, (m, width)))).astype(np.float32)
        elif kind == "sub_in_zero":
            s[:] = 0.0
            s[m // 2:m // 2 + 3] = _bits(rng.integers(0x1000, 0x800000, (3, width), dtype=np.uint32))
        elif kind == "lone_nzero":
            s[:] = -0.0
        elif kind == "lone_min":
            s[:] = _bits(1)
        elif kind == "inf_re":
            s[:, 0] = np.inf
        elif kind == "ninf_im":
            s[:, width - 1] = -np.inf
        elif kind == "nan":
            s[:] = _bits(0x7FC00000)
        elif kind == "inf_both":
            s[:] = np.inf
        elif kind == "overflow":
            s[:] = (np.float32(3.0e38) * np.where(np.arange(m) & 1, -1.0, 1.0)).astype(np.float32)[:, None]
    starts = [seg["start"] for seg in table]
    assert any(a & 1 for a in starts), "no segment starts at an odd sample"
    assert n <= BLOCK or any(seg["start"] < e <= seg["start"] + seg["len"] for seg in table for e in range(BLOCK, n, BLOCK)), \
        "no segment straddles an 8192-sample edge"
    return v.reshape(-1), table


U8_KINDS = ("silence", "floor", "ceiling", "around", "lone_silence")


def salt_u8(u8, lp, seed=0, every=1):
    """The u8 IQ analogue (interleaved, 2 bytes per sample): runs of 2 lp samples of byte 128 (converted: exactly +0), of 0, of 255,
    of 127 / 129 alternating, and a lone 128.  Same layout and table as salt."""
    u8 = np.array(u8, dtype=np.uint8, copy=True)
    n = u8.size // 2
    lengths = {k: 2 * lp for k in U8_KINDS[:4]}
    lengths["lone_silence"] = 1
    table = _layout(n, lp, list(U8_KINDS), lengths, every)
    v = u8.reshape(n, 2)
    for seg in table:
        a, m = seg["start"], seg["len"]
        kind = seg["kind"]
        if kind in ("silence", "lone_silence"):
            v[a:a + m] = 128
        elif kind == "floor":
            v[a:a + m] = 0
        elif kind == "ceiling":
            v[a:a + m] = 255
        else:
            odd = (np.arange(m)[:, None] + np.arange(2)[None, :]) & 1
            v[a:a + m] = np.where(odd, 129, 127)
    assert any(seg["start"] & 1 for seg in table)
    assert n <= BLOCK or any(seg["start"] < e <= seg["start"] + seg["len"] for seg in table for e in range(BLOCK, n, BLOCK))
    return v.reshape(-1), table


def awkward_taps(taps, level, last_zero=False):
    """Level 1: a few interior taps become +0.0 and -0.0; every nonzero tap stays at or above 2^-119 (a u8-fused kernel that scales its
    taps by 1/128 stays eligible); the last tap is kept (it must be nonzero) or, with last_zero, set to 0.0.  Level 2 additionally
    plants 1e-40 (a subnormal tap), -2^-125 and 1e30: a nonzero tap below 2^-119.  A half-tap set is treated the same way."""
    t = np.array(taps, dtype=np.float32, copy=True)
    n = t.size
    assert n >= 16 and level in (0, 1, 2)
    if level == 0:
        return t
    t[n // 3], t[n // 2], t[(2 * n) // 3] = 0.0, -0.0, 0.0
    if level == 2:
        t[n // 4] = np.float32(1e-40)
        t[n // 4 + 2] = -np.float32(2.0) ** -125
        t[(3 * n) // 4] = np.float32(1e30)
    if last_zero:
        t[-1] = 0.0
    elif t[-1] == 0:
        t[-1] = np.float32(0.001)
    nz = np.abs(t[t != 0])
    assert (level == 2) == bool((nz < 2.0 ** -119).any())
    return t


def nan_share(a):
    return float(np.isnan(np.asarray(a, np.float32)).mean()) if np.size(a) else 0.0


def classes_present(a):
    """Which of the four classes a float32 array holds: exact zeros, subnormals, infinities, NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32).ravel()
    mag = a.view(np.uint32) & 0x7FFFFFFF
    return {"zero": bool((mag == 0).any()), "subnormal": bool(((mag > 0) & (mag < 0x00800000)).any()),
            "inf": bool((mag == 0x7F800000).any()), "nan": bool((mag > 0x7F800000).any())}


def assert_not_vacuous(exp, what, need=("zero", "subnormal", "inf", "nan")):
    """On the CPU side alone: the expected output holds every class in `need` (a case that does not is changed, not waived)."""
    have = classes_present(exp)
    missing = [k for k in need if not have[k]]
    assert not missing, f"{what}: the expected output holds no {' / '.join(missing)} element -- the case does not test that class"


def assert_same_classes(got, exp, what, max_nan_share=0.10):
    """exp: the CPU side as an array (oracle, Pipes model).  got: the device's answer -- or, in the oracle-against-reference tests,
    the reference build's (an array, or its recorded digest).  The cap on exp's NaN share is a condition on the inputs, checked before
    `got` is looked at; then NaN positions must agree, and every other element bit for bit.  Returns the share."""
    exp = np.ascontiguousarray(exp, dtype=np.float32).ravel()
    share = nan_share(exp)
    print(f"{what}: NaN share of the expected output {share:.4f} ({exp.size} elements)")
    assert share <= max_nan_share, f"{what}: {share:.3f} of the expected output is NaN (cap {max_nan_share}): the input is over-salted"
    if isinstance(got, RecordedArray):
        assert got.canon, f"{what}: the recorded answer was not taken with NaNs made canonical"
        assert_bit_equal(got, exp, what)
        return share
    got = np.ascontiguousarray(got, dtype=np.float32).ravel()
    assert got.shape == exp.shape, f"{what}: {got.size} elements vs {exp.size}"
    gn, en = np.isnan(got), np.isnan(exp)
    bad = np.nonzero(gn != en)[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: NaN positions differ in {bad.size}/{exp.size} elements; first at {i}: got {got[i]!r} "
                             f"({got.view(np.uint32)[i]:#x}), expected {exp[i]!r} ({exp.view(np.uint32)[i]:#x})")
    assert_bit_equal(canonical_nan(got), canonical_nan(exp), what)
    return share


# ---- convertBladeRFTransmit (convert.c:87-101) ----------------------------------------------------------------------------------
def convert_tx_spec(x):
    """The restatement in integer arithmetic: val = (x + 1) * 2048 in float32; the int16 cast as x86 performs it (truncate to int32,
    keep the low 16 bits: the C cast itself wherever that is defined, |trunc val| < 2^15); minus 2048, kept in 16 bits; clamp.
    NaN and values that do not fit 32 bits -- undefined in C -- convert to 0x80000000, x86's "integer indefinite"."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        val = (x + np.float32(1)) * np.float32(2048)
    assert val.dtype == np.float32
    fits = np.abs(val) < 2.0 ** 31                       # False for NaN
    wide = np.where(fits, np.trunc(np.where(fits, val, 0)).astype(np.int64), -2 ** 31)
    res = wide.astype(np.int16)
    res = (res.astype(np.int32) - 2048).astype(np.int16)
    return np.clip(res, -2048, 2047).astype(np.int16)


def convert_tx_inputs():
    """(defined, wild): a dense sweep of [-17, 16) in steps of 2^-12 with +-0, subnormals, k/2048 -1 +- 1 ulp around the clamps and
    the ends of the nominal range [-1, 1]; and the arguments whose int16 cast is undefined behaviour in C (the kernel claims x86's)."""
    sweep = (np.arange(-17 * 4096, 16 * 4096, dtype=np.int64) / 4096.0).astype(np.float32)
    specials = [0.0, -0.0, 1e-40, -1e-40, -1.0, 1.0, 1.0 - 2.0 ** -24]
    near = []
    for k in list(range(-4, 5)) + list(range(2044, 2052)) + list(range(4092, 4100)) + [32767, 32768, 32769, -32767, -32768]:
        c = np.float32(k / 2048.0 - 1.0)
        near += [c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))]
    defined = np.concatenate([sweep, _bits([1, 0x80000001, 0x007FFFFF, 0x807FFFFF]), np.array(specials + near, np.float32)])
    wild = np.array([1e6, -1e6, 3e9, -3e9, np.inf, -np.inf, np.nan], np.float32)
    return defined, wild


SCALE_FACTORS = (0.2, 0.0, -0.0, 1e-30, 3e38)
