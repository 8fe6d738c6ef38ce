"""The case table of the AM bank's tests reaches what it is there for -- shown from the models alone (tests/am_bank_cases.py), without
the product: conditions on the inputs, not measurements of the code under test."""
import numpy as np

import am_bank_cases as AC
import tuner_bank_cases as BC
import test_gpu_tuner as T


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_tile_size_is_read_from_the_code():
    assert AC.OUTS == 512 and AC.COUNTS == [1, 511, 512, 513, 1535]


def test_every_seamed_case_has_cross_outputs_that_show_in_the_envelope(oracle):
    """Seamed runs start at output K0_CROSS: each count's range holds straddlers, and for at least one of them the envelope of the
    Cross-order sum differs from the envelope of the One-order sum -- in EVERY channel for the one-output run, so no row could pass
    with the One order there."""
    cross = BC.straddlers(AC.B, AC.K_ALL)
    assert cross[0] == AC.K0_CROSS
    for fmt in AC.FORMATS:
        for nch in (1, 3, 32):
            for j, t in enumerate(BC.bank_tables(nch)):
                seamed, plain = AC.expected_env(oracle, t, AC.B, fmt), AC.expected_env(oracle, t, 0, fmt)
                diff = np.nonzero(_bits(seamed) != _bits(plain))[0]
                assert diff.size and set(diff) <= set(cross), f"{fmt}, {nch} channels, channel {j}"
                for count in AC.COUNTS:
                    inside = cross[(cross >= AC.K0_CROSS) & (cross < AC.K0_CROSS + count)]
                    assert inside.size >= 1
                    if count > 1:
                        assert np.isin(diff, inside).any(), f"{fmt}, {nch} channels, channel {j}, {count} outputs: no Cross output shows"
            # the one-output run: some channel of each bank shows its Cross order
            assert any(_bits(AC.expected_env(oracle, t, AC.B, fmt))[AC.K0_CROSS] != _bits(AC.expected_env(oracle, t, 0, fmt))[AC.K0_CROSS]
                       for t in BC.bank_tables(nch)), f"{fmt}, {nch} channels: output {AC.K0_CROSS} shows no Cross order"
        # the cut runs: every launch behind the first cut that holds straddlers shows one, in the audio behind dcBlocker too
        edges = [0] + AC.ODD_CUTS + [AC.K_ALL]
        t = BC.bank_tables(1)[0]
        a, p = AC.expected_audio(oracle, t, AC.B, fmt)[0], AC.expected_audio(oracle, t, 0, fmt)[0]
        assert (_bits(a) != _bits(p)).any()
        assert sum(((cross >= lo) & (cross < hi)).any() for lo, hi in zip(edges[:-1], edges[1:])) >= 3


def test_subnormal_case(oracle):
    """The sparse stream against the subnormal / -0 table: envelope inputs with subnormal parts, envelopes that are subnormal, and
    envelopes that are +0 (from (+-0, +-0))."""
    iq = AC.sparse_expected_iq(oracle, BC.SUBNORMALS, AC.B)
    tiny = np.float32(np.finfo(np.float32).tiny)
    parts = np.abs(iq)
    assert ((parts > 0) & (parts < tiny)).sum() > 100, "no subnormal part under the magnitude"
    env = AC.envelope(iq)
    assert ((env > 0) & (env < tiny)).sum() > 50
    zero = np.nonzero(_bits(env) == 0)[0]
    assert zero.size > 100, "no +0 envelope"
    assert (_bits(env) != 0x80000000).all(), "magnitude never gives -0"
    pairs = iq.reshape(-1, 2)[zero]
    assert ((pairs != 0).any(axis=1)).any(), "no +0 envelope of a subnormal part beside a zero (exponent 0 = 0: its square underflows)"
    assert ((pairs == 0).all(axis=1)).any(), "no +0 envelope of (0, 0)"
    assert AC.sparse_expected_iq(oracle, BC.SUBNORMALS, AC.B).size == 2 * AC.SPARSE_OUT


def test_nonfinite_case(oracle):
    """One +Inf and one NaN sample: +Inf envelopes in the windows of the first, NaN envelopes in the windows of the second, finite
    elsewhere; behind dcBlocker everything from the second +Inf envelope on is NaN."""
    t = T.osc_table(1000)
    env, audio = AC.nonfinite_expected(oracle, t, AC.B, False), AC.nonfinite_expected(oracle, t, AC.B, True)
    w_inf, w_nan = AC.window_outputs(AC.INF_AT), AC.window_outputs(AC.NAN_AT)
    assert w_inf.size == 16 and w_nan.size == 16 and w_inf[-1] < w_nan[0]
    assert (_bits(env[w_inf]) == 0x7F800000).all(), "+Inf envelopes at the windows of the Inf sample"
    assert np.isnan(env[w_nan]).all()
    rest = np.ones(env.size, bool)
    rest[w_inf] = rest[w_nan] = False
    assert np.isfinite(env[rest]).all()
    assert np.isfinite(audio[:w_inf[0]]).all() and _bits(audio)[w_inf[0]] == 0x7F800000
    assert np.isnan(audio[w_inf[0] + 1:]).all(), "Inf - Inf: NaN from there on"


def test_carried_dc_states_are_nonzero_and_differ_between_channels(oracle):
    for fmt in AC.FORMATS:
        for nch in (3, 32):
            tables = BC.bank_tables(nch)
            for k in AC.ODD_CUTS + [AC.K0_CROSS, AC.K_ALL]:
                st = np.array([AC.state_before(oracle, t, AC.B, fmt, k) for t in tables])
                assert (st != 0).all(), f"{fmt}: a zero state at output {k}"
                assert len({s.tobytes() for s in st}) == len({t.tobytes() for t in tables}), f"{fmt}: two tables share a state at output {k}"
                assert all(a.tobytes() != b.tobytes() for a, b in zip(st[:-1], st[1:])), f"{fmt}: neighbours share a state at output {k}"
    # and the state is what the model's dcBlocker continues from: the stream cut at a state equals the stream
    t = BC.bank_tables(1)[0]
    env, (audio, fs, fo) = AC.expected_env(oracle, t, AC.B, "u8"), AC.expected_audio(oracle, t, AC.B, "u8")
    s = AC.state_before(oracle, t, AC.B, "u8", 1009)
    y, fs2, fo2 = oracle.dc_blocker(env[1009:], float(s[0]), float(s[1]))
    assert np.array_equal(_bits(y), _bits(audio[1009:])) and (np.float32(fs2), np.float32(fo2)) == (fs, fo)
    assert np.array_equal(AC.state_before(oracle, t, AC.B, "u8", AC.K_ALL), np.array([fs, fo], np.float32))
