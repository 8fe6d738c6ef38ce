// descriptors.hpp -- the device-side twins of the reference's Filter / Decimator /
// Resampler records (hs_sources/SDR/Filter.hs:116-144) with their taps prepared the
// way the reference's constructors prepare them (A10: Filter.hs:146-148,163-175,
// 234-245,277-290,317-331,408-425; FilterInternal.hs:277-319).
#pragma once
#include <vector>

#include "common.hpp"
#include "kernels.hpp"

namespace sdrhip {

struct FirDesc {
    int order = SDRHIP_ORDER_AVX;
    bool cplx = false;
    bool sym = false;
    int factor = 1;       // decimation (1 = filter)
    int Lp = 0;           // numCoeffsF / numCoeffsD: what the Pipe sees
    int lanes = 8;        // real data lane count
    ComplexOrder corder = CO_L4;
    int ntaps_kernel = 0; // length of d_taps as the kernel consumes it
    // Device copies are made on first use (ensure_device), so descriptors -- and the
    // planning arithmetic built on them -- can be created on a host without a GPU.
    mutable int device = -1;           // the device the taps were uploaded to (-1: not yet)
    mutable float* d_taps = nullptr;   // real: padded plain (or half for sym); complex RC: duplicated
    mutable float* d_cross = nullptr;  // Lp plain taps for the sequential Cross outputs
    mutable float* d_plain = nullptr;  // padded plain taps (aliases d_cross)
    mutable float* d_scaled = nullptr; // complex stages: plain taps / 128 for the u8-fused tiled kernel (null: some tap too small to scale exactly)
    std::vector<float> h_scaled;
    std::vector<float> h_plain;        // Lp plain taps (sym: c ++ reverse c)
    std::vector<float> h_kernel;       // what d_taps holds
    // tap Lp-1 is the zero the constructor padded the filter with (lets the u8 kernels skip its MACs)
    bool last_tap_is_padding() const { return (int)h_plain.size() == Lp && h_plain[Lp - 1] == 0.0f; }
    int ensure_device() const;
    ~FirDesc();
};

struct ResampDesc {
    int order = SDRHIP_ORDER_AVX;
    bool cplx = false;
    int I = 1, D = 1;
    int Lp = 0;           // numCoeffsR = roundUp(ntaps, I * simd)
    int lanes = 8;
    ComplexOrder corder = CO_X4;
    int ntaps = 0;        // unpadded
    int num_coeffs = 0;   // longest group, unpadded
    int num_groups = 0;
    int row_stride = 0;   // padded group length
    int nloop = 0;        // floats the SIMD loop actually walks
    std::vector<int> increments, offsets, lut;  // lut: filter offset -> group
    std::vector<float> h_groups, h_plain;
    mutable int device = -1;           // the device the taps were uploaded to (-1: not yet)
    mutable float* d_groups = nullptr;
    mutable float* d_plain = nullptr;
    mutable int* d_ext = nullptr;      // more than 64 groups: prefix sums of the increments + filter offsets (kernels.hpp ResampTable::ext)
    int ensure_device() const;
    int64_t in_offset(int64_t m) const { return ceil_div64(m * (int64_t)D, I); }
    int filter_offset(int64_t m) const { return (int)(in_offset(m) * I - m * (int64_t)D); }
    int group(int64_t m) const { return lut[filter_offset(m)]; }
    ~ResampDesc();
};

// polyphase split, FilterInternal.hs:297-319
void prepare_coeffs(int n, int I, int D, const float* coeffs, int ncoeffs, int& num_coeffs, int& row_stride,
                    std::vector<int>& increments, std::vector<int>& offsets, std::vector<float>& groups);

int fir_create(FirDesc* d, int order, bool cplx, int factor, const float* coeffs, int ncoeffs);
int fir_sym_create(FirDesc* d, int order, int factor, const float* half, int nhalf);
// gain: applied to every output after the filter's own rounding (a separate f32 multiply,
// exactly what `P.map (VG.map (* g))` after the Pipe computes); 1.0f = none.
int fir_run(const FirDesc* d, hipStream_t s, const void* d_in, bool in_u8, int64_t in_base, float* d_out,
            int64_t k_begin, int64_t k_end, int64_t seam_block, float gain = 1.0f);

int resamp_create(ResampDesc* r, int order, bool cplx, int I, int D, const float* coeffs, int ncoeffs);
// out_block: the Pipe's output block size (blockSizeOut; 0 = unbounded) -- it decides one corner case of the seam
// classification (kernels.hpp: late_output_is_one)
int resamp_run(const ResampDesc* r, hipStream_t s, const float* d_in, int64_t in_base, float* d_out,
               int64_t k_begin, int64_t k_end, int64_t seam_block, int64_t out_block = 0);
// fmDemod + resampler: d_iq = the decimator output whose phase step (fmDemod, Demod.hs:21-46) is input `in_base`, y_count
// inputs; d_in = the buffer the stand-alone fmDemod would fill (abi_device.cpp)
int resamp_run_demod(const ResampDesc* r, hipStream_t s, const float* d_iq, bool iq_has_prev, int64_t y_count, const float* d_in,
                     int64_t in_base, float* d_out, int64_t k_begin, int64_t k_end, int64_t seam_block, int64_t out_block,
                     bool* demod_fused);

// abi_fir_rows.cpp: does the banked route of the row forms (sdrhip_*_run_rows, route 1) serve outputs [k_begin, k_end) of `rows` rows
// of this descriptor?  Host arithmetic (the plan sdrhip_debug_fir_rows_plan reports), for callers that pick the route themselves.
bool fir_rows_banked(const FirDesc* d, int rows, int64_t k_begin, int64_t k_end, int64_t seam_block);
bool resamp_rows_banked(const ResampDesc* r, int rows, int64_t k_begin, int64_t k_end, int64_t seam_block);

// The tuner (include/sdr_hip.h): a complex decimator's prepared taps plus the oscillator table.  Immutable after create except for
// the route and the scratch lanes of the two-pass route, so host threads may share one.
// (its input format: InFmt, kernels.hpp)
struct TunerScratch;
struct TunerDesc {
    FirDesc fir;                       // as sdrhip_decimator_create(order, data_complex = 1, ...) prepares it
    int period = 0;
    std::vector<float> h_osc;          // period (re, im) pairs
    mutable float* d_osc = nullptr;
    mutable int route = 0;             // 0 = auto, 1 = fused, 2 = two-pass
    TunerScratch* scratch = nullptr;   // tuner.cpp
    int ensure_device() const;
    TunerDesc();
    ~TunerDesc();
    TunerDesc(const TunerDesc&) = delete;
    TunerDesc& operator=(const TunerDesc&) = delete;
};
int tuner_run(const TunerDesc* t, hipStream_t s, const void* d_in, InFmt fmt, int64_t in_base, float* d_out, int64_t k_begin,
              int64_t k_end, int64_t seam_block);

// The tuner bank (include/sdr_hip.h): K tuners of the same decimator over one input.  The bank OWNS those K tuner descriptors -- they
// ARE the channel-by-channel route -- and, for the banked launch (kernels_tuner_bank.hip), one device copy of all the tables back to
// back; the banked launch takes its taps from channel 0's FirDesc (every channel's are the same).  Immutable after create except for
// the route, so host threads may share one.
struct TunerBankDesc {
    std::vector<TunerDesc*> ch;                // channel j as a tuner
    std::vector<float> h_tables;               // every table, back to back
    int off[kTunerBankMaxChannels] = {0};      // channel j's first (re, im) pair in h_tables / d_tables
    int period[kTunerBankMaxChannels] = {0};
    mutable float* d_tables = nullptr;         // made by the first banked run
    mutable int route = 0;                     // 0 = auto, 1 = banked, 2 = channel by channel
    int ensure_device() const;                 // channel 0's taps and the tables
    TunerBankDesc() = default;
    ~TunerBankDesc();
    TunerBankDesc(const TunerBankDesc&) = delete;
    TunerBankDesc& operator=(const TunerBankDesc&) = delete;
};
int tuner_bank_run(const TunerBankDesc* b, hipStream_t s, const void* d_in, InFmt fmt, int64_t in_base, float* d_out, int64_t out_stride,
                   int64_t k_begin, int64_t k_end, int64_t seam_block);

// ---- the output forms of the bank family (tuner_bank.cpp) ---------------------------------------------------------------------------
// What the bank's kernel pair (kernels_tuner_bank.hip) stores for a finished output: the complex value (rows of 2 floats per output,
// 8-byte aligned, an even stride), its envelope, or fmDemod's phase against the output before it (rows of 1 float per output at any
// float address).  The phase form reads every channel's output k_begin - 1 from d_state (channels (re, im) pairs) and leaves output
// k_end - 1 in d_final; the two do not overlap.
struct BankForm {
    enum Kind { IQ, ENV, PHASE } kind = IQ;
    const float* d_state = nullptr;
    float* d_final = nullptr;
    bool state_overlaps(int channels) const;
};
inline int64_t row_floats(int64_t count) { return (count + 3) & ~(int64_t)3; }   // workspace rows start 16-byte aligned
// channel 0's decimator over outputs [k_begin, k_end) (ranges and taps are the same for every channel)
Geom bank_geom(const FirDesc* d, int64_t in_base, int64_t k_begin, int64_t k_end, int64_t seam_block);
// whether the fused launch (set) takes this range in this form; d_out: the complex rows of the IQ form (the float forms ignore it)
bool bank_fused_fits(const TunerBankDesc* tb, const Geom& g, const void* d_in, InFmt fmt, const BankForm& form, const float* d_out);
// The steps the bank objects and the banks' Pipes are built from; row j of a form is at d_out + j * out_stride floats.
// bank_fused: the fused launch (set); SDRHIP_OK = launched, kBankNotThisShape = nothing launched, negative = an error.
// bank_composed (the float forms): the tuner bank into d_iq (channels rows of 2 * row_floats(count) floats, 16-byte aligned), then
// amDemod's or fmDemod's rows form, through the C ABI as a caller without the bank objects makes the calls.
// bank_cross: every output Cross, one launch for all channels (the ragged pushes of the banks' Pipes), no route and no auto rule.
// bank_form_run: what the Pipes of the float forms run for the outputs inside a block -- bank_fused where bank_fused_fits says so,
// else bank_composed (d_iq null = no fall-back: SDRHIP_ERR_ARG).
constexpr int kBankNotThisShape = 1;
int bank_fused(const TunerBankDesc* tb, hipStream_t s, const Geom& g, const void* d_in, InFmt fmt, const BankForm& form, float* d_out,
               int64_t out_stride);
int bank_composed(const TunerBankDesc* tb, hipStream_t s, const void* d_in, InFmt fmt, int64_t in_base, float* d_out, int64_t out_stride,
                  int64_t k_begin, int64_t k_end, int64_t seam_block, const BankForm& form, float* d_iq);
int bank_cross(const TunerBankDesc* tb, hipStream_t s, const void* d_in, InFmt fmt, int64_t in_base, float* d_out, int64_t out_stride,
               int64_t k_begin, int64_t k_end, const BankForm& form);
int bank_form_run(const TunerBankDesc* tb, hipStream_t s, const void* d_in, InFmt fmt, int64_t in_base, float* d_out, int64_t out_stride,
                  int64_t k_begin, int64_t k_end, int64_t seam_block, const BankForm& form, float* d_iq);

// The AM bank (include/sdr_hip.h, am_bank.cpp): a BORROWED tuner bank, the envelope of each of its rows and, with dc_block, dcBlocker.
struct AmBankDesc {
    const TunerBankDesc* tb = nullptr;
    int dc_block = 0;
    mutable int route = 0;                     // 0 = auto, 1 = fused, 2 = composed
};

// The narrow-band FM bank (include/sdr_hip.h, nfm_bank.cpp): a BORROWED tuner bank and fmDemod of each of its rows.
struct NfmBankDesc {
    const TunerBankDesc* tb = nullptr;
    mutable int route = 0;                     // 0 = auto, 1 = fused, 2 = composed
};

// The narrow-channel bank (include/sdr_hip.h, narrow_bank.cpp): a BORROWED tuner bank, a BORROWED complex second decimator, the
// demodulator (NarrowForm, kernels.hpp) and, with the envelope form, dcBlocker.
struct NarrowBankDesc {
    const TunerBankDesc* tb = nullptr;
    const FirDesc* d2 = nullptr;
    int form = NARROW_ENV;
    int dc_block = 0;
    mutable int route = 0;                     // 0 = auto, 1 = fused, 2 = composed
};
// narrow_bank.cpp: everything behind the tuner bank over complex rows that exist (row j at d_rows + j * stride floats, element 0 =
// stage-1 output in_base, n_in readable): ONE k_narrow_rows launch where `fused` (narrow_stage2_fits says whether it may be), else
// the decimator's and the demodulator's rows forms; then dcBlocker's.  A caller that passes fused has made d2->ensure_device().  ws: narrow_stage2_bytes, 16-byte aligned.
size_t narrow_stage2_bytes(const NarrowBankDesc* b, int K, int64_t count, bool fused);
bool narrow_stage2_fits(const NarrowBankDesc* b, int K, const float* d_rows, int64_t stride, int64_t in_base, int64_t k_begin, int64_t k_end,
                        int64_t seam_block2);
int narrow_stage2(const NarrowBankDesc* b, hipStream_t s, bool fused, const float* d_rows, int64_t stride, int64_t in_base, int64_t n_in,
                  float* d_out, int64_t out_stride, int64_t k_begin, int64_t k_end, int64_t seam_block2, const float* d_state, float* d_final,
                  float* d_dc_state, float* ws, size_t ws_bytes);

}  // namespace sdrhip

struct sdrhip_am_bank : sdrhip::AmBankDesc {};
struct sdrhip_nfm_bank : sdrhip::NfmBankDesc {};
struct sdrhip_narrow_bank : sdrhip::NarrowBankDesc {};
struct sdrhip_filter : sdrhip::FirDesc {};
struct sdrhip_decimator : sdrhip::FirDesc {};
struct sdrhip_resampler : sdrhip::ResampDesc {};
struct sdrhip_tuner : sdrhip::TunerDesc {};
struct sdrhip_tuner_bank : sdrhip::TunerBankDesc {};
