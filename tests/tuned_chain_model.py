"""The FM receiver with a tuner, restated: oracle/pipes_model.py's fm_receiver with one more stage.  TEST INFRASTRUCTURE ONLY.

    P.map convert >-> P.map (VG.zipWith (*) osc) >-> firDecimator deci samples >-> fmDemod >-> firResampler resp samples
                  >-> firFilter filt samples >-> P.map (* gain)

The source delivers `block`-sample buffers and buffer i starts at absolute stream index i * block, so the oscillator of
buffer i is the table rotated to (i * block) mod period: tuner_model.mix(buffer, osc, pos0 = i * block) -- in general pos0 =
the number of samples in the buffers before it.  The (*) parity is
argued as for the tuner (tests/tuner_model.py); no GHC ran."""
import tuner_model as TM
from oracle import pipes_model as PM


def fm_receiver_tuned(oracle, u8_blocks, osc_iq, decim_taps, factor, resamp_taps, I, D, audio_half, gain=None, block=8192,
                      order=PM.ORDER_AVX, mix_whole_stream=False):
    """u8_blocks: the source's buffers of interleaved u8 IQ, the first at stream index 0 -> the audio blocks; block = the
    blockSizeOut of the four Pipes, as in PM.fm_receiver (fm.hs uses one number, `samples`, for both).
    mix_whole_stream: mix the concatenated stream once and cut it again (the same samples by another route: a check of the
    model's own phase bookkeeping)."""
    iq = [oracle.convert_u8(b) for b in u8_blocks]                                      # P.map convert
    if mix_whole_stream:
        import numpy as np
        whole = TM.mix(np.concatenate(iq), osc_iq, 0)
        edges = np.cumsum([0] + [b.size for b in iq])
        mixed = [whole[a:b] for a, b in zip(edges[:-1], edges[1:])]
    else:
        mixed, pos = [], 0
        for b in iq:                                                                    # P.map (VG.zipWith (*) osc)
            mixed.append(TM.mix(b, osc_iq, pos))
            pos += b.size // 2
    deci = PM.FilterModel(oracle, decim_taps, order, complex_=True, factor=factor)
    d_blocks, _ = PM.fir_decimator_pipe(deci, mixed, block)                             # firDecimator deci samples
    y_blocks = PM.fm_demod_pipe(oracle, d_blocks)                                       # fmDemod
    resp = PM.ResamplerModel(oracle, I, D, resamp_taps, order)
    z_blocks, _ = PM.fir_resampler_pipe(resp, y_blocks, block)                          # firResampler resp samples
    filt = PM.FilterModel(oracle, audio_half, order, sym=True)
    a_blocks, _ = PM.fir_filter_pipe(filt, z_blocks, block)                             # firFilter filt samples
    if gain is not None:
        a_blocks = [oracle.scale(gain, a) for a in a_blocks]                            # P.map (VG.map (* gain))
    return a_blocks
