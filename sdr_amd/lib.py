"""ctypes binding of libsdr_hip.so -- the ONLY way Python reaches the product.

There is no CPU fallback: if the HIP library is missing or fails to load, import
of this module raises.  (The CPU oracle lives under oracle/ and is never imported
from here.)
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libsdr_hip.so")

ORDER_SCALAR, ORDER_SSE, ORDER_AVX = 0, 1, 2

_f32p = C.POINTER(C.c_float)
_u8p = C.POINTER(C.c_uint8)
_i16p = C.POINTER(C.c_int16)
_i32p = C.POINTER(C.c_int)
_vp = C.c_void_p
_i64 = C.c_int64


class SdrHipError(RuntimeError):
    pass


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own copy of libamdhip64 / libhsa-runtime64 and looks it up by
    file name, libsdr_hip.so asks for the system copy by SONAME; whichever loads second then brings a second runtime into
    the process and loses the GPU ("no ROCm-capable device").  If torch is installed, map ITS copies first (by path, without
    importing torch): our library's SONAME lookup then resolves to them, and a later `import torch` finds the very same
    files already mapped.  Without torch (a plain C host program, examples/fm_replay.c) the system runtime is used."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                return


def _load():
    if not os.path.exists(LIB_PATH):
        raise SdrHipError(
            f"{LIB_PATH} not found: build it with `python -m sdr_amd.build` "
            "(there is deliberately no CPU fallback)")
    _share_torch_hip_runtime()
    return C.CDLL(LIB_PATH)


lib = _load()

# ---- signatures -----------------------------------------------------------------
lib.sdrhip_version.restype = C.c_char_p
lib.sdrhip_set_small_launch_outputs.argtypes = [C.c_int]
lib.sdrhip_set_small_launch_outputs.restype = C.c_int
lib.sdrhip_last_error.restype = C.c_char_p
lib.sdrhip_device_name.argtypes = [C.c_char_p, C.c_int]
lib.sdrhip_malloc.argtypes = [C.POINTER(_vp), C.c_size_t]
lib.sdrhip_free.argtypes = [_vp]
lib.sdrhip_malloc_host.argtypes = [C.POINTER(_vp), C.c_size_t]
lib.sdrhip_free_host.argtypes = [_vp]
for _n in ("sdrhip_memcpy_h2d", "sdrhip_memcpy_d2h", "sdrhip_memcpy_d2d"):
    getattr(lib, _n).argtypes = [_vp, _vp, C.c_size_t, _vp]
lib.sdrhip_stream_create.argtypes = [C.POINTER(_vp)]
lib.sdrhip_stream_destroy.argtypes = [_vp]
lib.sdrhip_stream_sync.argtypes = [_vp]

lib.sdrhip_filter_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int, _f32p, C.c_int]
lib.sdrhip_filter_sym_create.argtypes = [C.POINTER(_vp), C.c_int, _f32p, C.c_int]
lib.sdrhip_filter_num_coeffs.argtypes = [_vp]
lib.sdrhip_filter_destroy.argtypes = [_vp]
lib.sdrhip_filter_destroy.restype = None
lib.sdrhip_filter_run.argtypes = [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64]

lib.sdrhip_decimator_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, _f32p, C.c_int]
lib.sdrhip_decimator_sym_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int, _f32p, C.c_int]
lib.sdrhip_decimator_num_coeffs.argtypes = [_vp]
lib.sdrhip_decimator_factor.argtypes = [_vp]
lib.sdrhip_decimator_destroy.argtypes = [_vp]
lib.sdrhip_decimator_destroy.restype = None
lib.sdrhip_decimator_run.argtypes = [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64]
lib.sdrhip_decimator_run_u8.argtypes = [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64]

lib.sdrhip_tuner_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int, _f32p, C.c_int, _f32p, C.c_int]
lib.sdrhip_tuner_num_coeffs.argtypes = [_vp]
lib.sdrhip_tuner_factor.argtypes = [_vp]
lib.sdrhip_tuner_period.argtypes = [_vp]
lib.sdrhip_tuner_destroy.argtypes = [_vp]
lib.sdrhip_tuner_destroy.restype = None
lib.sdrhip_tuner_run.argtypes = [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64]
lib.sdrhip_tuner_run_u8.argtypes = [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64]
lib.sdrhip_tuner_run_i16.argtypes = [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64]
lib.sdrhip_debug_tuner_i16_launches.argtypes = []
lib.sdrhip_debug_tuner_i16_launches.restype = C.c_longlong
lib.sdrhip_tuner_set_route.argtypes = [_vp, C.c_int]
lib.sdrhip_tuner_shift_table.argtypes = [_i64, _i64, _f32p]
lib.sdrhip_debug_tuner_fused_launches.argtypes = []
lib.sdrhip_debug_tuner_fused_launches.restype = C.c_longlong
lib.sdrhip_debug_set_tuner_chunk.argtypes = [_i64]
lib.sdrhip_debug_set_tuner_chunk.restype = _i64
lib.sdrhip_tuner_bank_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int, _f32p, C.c_int, C.c_int, C.POINTER(_f32p), C.POINTER(C.c_int)]
lib.sdrhip_tuner_bank_destroy.argtypes = [_vp]
lib.sdrhip_tuner_bank_destroy.restype = None
lib.sdrhip_tuner_bank_channels.argtypes = [_vp]
lib.sdrhip_tuner_bank_period.argtypes = [_vp, C.c_int]
lib.sdrhip_tuner_bank_num_coeffs.argtypes = [_vp]
lib.sdrhip_tuner_bank_factor.argtypes = [_vp]
lib.sdrhip_tuner_bank_run.argtypes = [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64]
lib.sdrhip_tuner_bank_run_u8.argtypes = [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64]
lib.sdrhip_tuner_bank_run_i16.argtypes = [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64]
lib.sdrhip_tuner_bank_set_route.argtypes = [_vp, C.c_int]
lib.sdrhip_debug_tuner_bank_launches.argtypes = []
lib.sdrhip_debug_tuner_bank_launches.restype = C.c_longlong
lib.sdrhip_debug_tuner_bank_cross_launches.argtypes = []
lib.sdrhip_debug_tuner_bank_cross_launches.restype = C.c_longlong
lib.sdrhip_am_bank_create.argtypes = [C.POINTER(_vp), _vp, C.c_int]
lib.sdrhip_am_bank_destroy.argtypes = [_vp]
lib.sdrhip_am_bank_destroy.restype = None
lib.sdrhip_am_bank_channels.argtypes = [_vp]
lib.sdrhip_am_bank_set_route.argtypes = [_vp, C.c_int]
lib.sdrhip_am_bank_workspace_bytes.argtypes = [_vp, _i64]
lib.sdrhip_am_bank_workspace_bytes.restype = C.c_size_t
for _n in ("sdrhip_am_bank_run", "sdrhip_am_bank_run_u8", "sdrhip_am_bank_run_i16"):
    getattr(lib, _n).argtypes = [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _vp, _vp, C.c_size_t]
lib.sdrhip_debug_am_bank_launches.argtypes = []
lib.sdrhip_debug_am_bank_launches.restype = C.c_longlong
lib.sdrhip_debug_am_bank_fixup_launches.argtypes = []
lib.sdrhip_debug_am_bank_fixup_launches.restype = C.c_longlong
lib.sdrhip_debug_am_bank_cross_launches.argtypes = []
lib.sdrhip_debug_am_bank_cross_launches.restype = C.c_longlong
lib.sdrhip_nfm_bank_create.argtypes = [C.POINTER(_vp), _vp]
lib.sdrhip_nfm_bank_destroy.argtypes = [_vp]
lib.sdrhip_nfm_bank_destroy.restype = None
lib.sdrhip_nfm_bank_channels.argtypes = [_vp]
lib.sdrhip_nfm_bank_set_route.argtypes = [_vp, C.c_int]
lib.sdrhip_nfm_bank_workspace_bytes.argtypes = [_vp, _i64]
lib.sdrhip_nfm_bank_workspace_bytes.restype = C.c_size_t
for _n in ("sdrhip_nfm_bank_run", "sdrhip_nfm_bank_run_u8", "sdrhip_nfm_bank_run_i16"):
    getattr(lib, _n).argtypes = [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, C.c_size_t]
lib.sdrhip_debug_nfm_bank_launches.argtypes = []
lib.sdrhip_debug_nfm_bank_launches.restype = C.c_longlong
lib.sdrhip_debug_nfm_bank_cross_launches.argtypes = []
lib.sdrhip_debug_nfm_bank_cross_launches.restype = C.c_longlong
lib.sdrhip_narrow_bank_create.argtypes = [C.POINTER(_vp), _vp, _vp, C.c_int, C.c_int]
lib.sdrhip_narrow_bank_destroy.argtypes = [_vp]
lib.sdrhip_narrow_bank_destroy.restype = None
lib.sdrhip_narrow_bank_channels.argtypes = [_vp]
lib.sdrhip_narrow_bank_set_route.argtypes = [_vp, C.c_int]
lib.sdrhip_narrow_bank_workspace_bytes.argtypes = [_vp, _i64]
lib.sdrhip_narrow_bank_workspace_bytes.restype = C.c_size_t
lib.sdrhip_narrow_bank_stage1_range.argtypes = [_vp, _i64, _i64, C.POINTER(_i64), C.POINTER(_i64)]
for _n in ("sdrhip_narrow_bank_run", "sdrhip_narrow_bank_run_u8", "sdrhip_narrow_bank_run_i16"):
    getattr(lib, _n).argtypes = [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, C.c_size_t]
lib.sdrhip_debug_narrow_bank_launches.argtypes = []
lib.sdrhip_debug_narrow_bank_launches.restype = C.c_longlong
lib.sdrhip_debug_narrow_bank_tile.argtypes = [C.c_int]

lib.sdrhip_resampler_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, C.c_int, _f32p, C.c_int]
lib.sdrhip_resampler_num_coeffs.argtypes = [_vp]
lib.sdrhip_resampler_num_groups.argtypes = [_vp]
lib.sdrhip_resampler_destroy.argtypes = [_vp]
lib.sdrhip_resampler_destroy.restype = None
lib.sdrhip_resampler_in_offset.argtypes = [_vp, _i64]
lib.sdrhip_resampler_in_offset.restype = _i64
lib.sdrhip_resampler_filter_offset.argtypes = [_vp, _i64]
lib.sdrhip_resampler_group.argtypes = [_vp, _i64]
lib.sdrhip_resampler_run.argtypes = [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64]

lib.sdrhip_convert_u8_run.argtypes = [_vp, _vp, _vp, _i64]
lib.sdrhip_convert_i16_run.argtypes = [_vp, _vp, _vp, _i64]
lib.sdrhip_scale_run.argtypes = [_vp, C.c_float, _vp, _vp, _i64]
lib.sdrhip_fm_demod_run.argtypes = [_vp, _vp, _i64, _vp, _i64, _i64, C.c_float, C.c_float]

lib.sdrhip_fm_chain_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int, _f32p, C.c_int, C.c_int, C.c_int, _f32p,
                                       C.c_int, _f32p, C.c_int, C.c_float, _i64]
lib.sdrhip_fm_chain_destroy.argtypes = [_vp]
lib.sdrhip_fm_chain_destroy.restype = None
lib.sdrhip_fm_chain_plan.argtypes = [_vp, _i64, _i64, _i64, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]
lib.sdrhip_fm_chain_ready.argtypes = [_vp, _i64]
lib.sdrhip_fm_chain_ready.restype = _i64
lib.sdrhip_fm_chain_max_halo.argtypes = [_vp]
lib.sdrhip_fm_chain_max_halo.restype = _i64
lib.sdrhip_fm_chain_workspace_bytes.argtypes = [_vp, _i64]
lib.sdrhip_fm_chain_workspace_bytes.restype = C.c_size_t
lib.sdrhip_fm_chain_run.argtypes = [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, C.c_size_t]

lib.sdrhip_fm_chain_graph_create.argtypes = [C.POINTER(_vp), _vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, C.c_size_t]
lib.sdrhip_fm_chain_graph_launch.argtypes = [_vp, _vp]
lib.sdrhip_fm_chain_graph_destroy.argtypes = [_vp]
lib.sdrhip_fm_chain_graph_destroy.restype = None
lib.sdrhip_fm_chain_set_overlap.argtypes = [_vp, C.c_int]
lib.sdrhip_fm_chain_join.argtypes = [_vp, _vp]
lib.sdrhip_fm_chain_set_fused_tail.argtypes = [_vp, C.c_int]
lib.sdrhip_fm_chain_set_small_chain.argtypes = [_vp, C.c_int, _i64, C.c_int]
lib.sdrhip_debug_small_chain_launches.restype = C.c_longlong
lib.sdrhip_fm_chain_set_tuner.argtypes = [_vp, _f32p, C.c_int]
lib.sdrhip_fm_chain_tuner_period.argtypes = [_vp]
lib.sdrhip_debug_small_chain_tuned_launches.argtypes = []
lib.sdrhip_debug_small_chain_tuned_launches.restype = C.c_longlong
lib.sdrhip_fm_bank_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int, _f32p, C.c_int, C.c_int, C.c_int, _f32p, C.c_int, _f32p, C.c_int,
                                      C.c_float, _i64, C.c_int, C.POINTER(_f32p), C.POINTER(C.c_int)]
lib.sdrhip_fm_bank_destroy.argtypes = [_vp]
lib.sdrhip_fm_bank_destroy.restype = None
lib.sdrhip_fm_bank_stations.argtypes = [_vp]
lib.sdrhip_fm_bank_period.argtypes = [_vp, C.c_int]
lib.sdrhip_fm_bank_plan.argtypes = [_vp, _i64, _i64, _i64, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]
lib.sdrhip_fm_bank_ready.argtypes = [_vp, _i64]
lib.sdrhip_fm_bank_ready.restype = _i64
lib.sdrhip_fm_bank_max_halo.argtypes = [_vp]
lib.sdrhip_fm_bank_max_halo.restype = _i64
lib.sdrhip_fm_bank_workspace_bytes.argtypes = [_vp, _i64]
lib.sdrhip_fm_bank_workspace_bytes.restype = C.c_size_t
lib.sdrhip_fm_bank_run.argtypes = [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, C.c_size_t]
lib.sdrhip_fm_bank_set_route.argtypes = [_vp, C.c_int, _i64, C.c_int]
lib.sdrhip_debug_fm_bank_launches.argtypes = []
lib.sdrhip_debug_fm_bank_launches.restype = C.c_longlong
lib.sdrhip_fm_bank_run_i16.argtypes = [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, C.c_size_t]
lib.sdrhip_debug_fm_bank_i16_launches.argtypes = []
lib.sdrhip_debug_fm_bank_i16_launches.restype = C.c_longlong
lib.sdrhip_debug_fused_tail_launches.argtypes = []
lib.sdrhip_debug_fused_tail_launches.restype = C.c_longlong
lib.sdrhip_debug_resample_cycle_launches.restype = C.c_longlong
lib.sdrhip_debug_decimate_real16_launches.restype = C.c_longlong
lib.sdrhip_debug_systolic_launches.restype = C.c_longlong
lib.sdrhip_debug_systolic_plain_launches.restype = C.c_longlong
lib.sdrhip_debug_decimator_crossfix_launches.restype = C.c_longlong
lib.sdrhip_debug_fused_demod_launches.restype = C.c_longlong
lib.sdrhip_debug_generic_u8_launches.restype = C.c_longlong
lib.sdrhip_debug_set_systolic.argtypes = [C.c_int]
lib.sdrhip_debug_set_systolic.restype = None
lib.sdrhip_debug_systolic_plan.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
lib.sdrhip_debug_systolic_plan.restype = None
lib.sdrhip_fm_chain_enable_timing.argtypes = [_vp, C.c_int]
lib.sdrhip_fm_chain_read_timing.argtypes = [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int)]

lib.sdrhip_fm_chain_halo_samples.argtypes = [_vp]
lib.sdrhip_fm_chain_halo_samples.restype = _i64
lib.sdrhip_fm_chain_halo_exchange.argtypes = [_vp, _vp, _vp, _vp, _i64]
lib.sdrhip_fm_chain_halo_staging_bytes.argtypes = [_vp, C.c_int]
lib.sdrhip_fm_chain_halo_staging_bytes.restype = C.c_size_t
lib.sdrhip_fm_chain_halo_exchange_batch.argtypes = [_vp, _vp, _vp, _vp, _i64, C.c_size_t, C.c_int, _vp]
lib.sdrhip_comm_get_unique_id.argtypes = [C.c_char_p]
lib.sdrhip_comm_init_rank.argtypes = [C.POINTER(_vp), C.c_int, C.c_int, C.c_char_p]
lib.sdrhip_comm_init_local.argtypes = [C.POINTER(_vp), C.c_int, C.POINTER(C.c_int), C.c_int]
lib.sdrhip_comm_destroy.argtypes = [_vp]
lib.sdrhip_comm_destroy.restype = None
lib.sdrhip_comm_rank.argtypes = [_vp]
lib.sdrhip_comm_size.argtypes = [_vp]
lib.sdrhip_comm_transport.argtypes = [_vp]
lib.sdrhip_comm_transport.restype = C.c_char_p
lib.sdrhip_halo_exchange.argtypes = [_vp, _vp, _vp, _vp, C.c_size_t]
lib.sdrhip_halo_exchange_all.argtypes = [C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.c_size_t]
_f64p = C.POINTER(C.c_double)
lib.sdrhip_fft_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int, C.c_int]
lib.sdrhip_fft_destroy.argtypes = [_vp]
lib.sdrhip_fft_destroy.restype = None
lib.sdrhip_fft_size.argtypes = [_vp]
lib.sdrhip_fft_bins.argtypes = [_vp]
lib.sdrhip_fft_run.argtypes = [_vp, _f64p, _f64p]
lib.sdrhip_fft_run_device.argtypes = [_vp, _vp, _vp, _vp]
lib.sdrhip_spectrum_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, _f64p, C.c_int, C.c_double]
lib.sdrhip_spectrum_destroy.argtypes = [_vp]
lib.sdrhip_spectrum_destroy.restype = None
lib.sdrhip_spectrum_size.argtypes = [_vp]
lib.sdrhip_spectrum_window.argtypes = [_vp, _f64p]
lib.sdrhip_spectrum_run_device.argtypes = [_vp, _vp, _vp, _i64, _i64, C.c_int, _vp]
lib.sdrhip_spectrum_run.argtypes = [_vp, _vp, _i64, _i64, C.c_int, _vp]
lib.sdrhip_spectrum_set_route.argtypes = [_vp, C.c_int]
lib.sdrhip_debug_spectrum_fused_launches.argtypes = []
lib.sdrhip_debug_spectrum_fused_launches.restype = C.c_longlong
lib.sdrhip_debug_spectrum_hipfft_batches.argtypes = []
lib.sdrhip_debug_spectrum_hipfft_batches.restype = C.c_longlong
lib.sdrhip_spectrum_reduce_run_device.argtypes = [_vp, _vp, _vp, _i64, _i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _vp]
lib.sdrhip_spectrum_reduce_run.argtypes = [_vp, _vp, _i64, _i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _vp]
lib.sdrhip_spectrum_set_reduce_split.argtypes = [_vp, C.c_int]
lib.sdrhip_debug_spectrum_reduce_split_launches.argtypes = []
lib.sdrhip_debug_spectrum_reduce_split_launches.restype = C.c_longlong
lib.sdrhip_debug_spectrum_reduce_layer_launches.argtypes = []
lib.sdrhip_debug_spectrum_reduce_layer_launches.restype = C.c_longlong
lib.sdrhip_filter_one.argtypes = [_vp, C.c_int, _f32p, _f32p]
lib.sdrhip_filter_cross.argtypes = [_vp, C.c_int, _f32p, C.c_int, _f32p, C.c_int, _f32p]
lib.sdrhip_decimator_one.argtypes = [_vp, C.c_int, _f32p, _f32p]
lib.sdrhip_decimator_cross.argtypes = [_vp, C.c_int, _f32p, C.c_int, _f32p, C.c_int, _f32p]
lib.sdrhip_resampler_one.argtypes = [_vp, C.c_int, C.c_int, _f32p, C.c_int, _f32p]
lib.sdrhip_resampler_cross.argtypes = [_vp, C.c_int, C.c_int, _f32p, C.c_int, _f32p, C.c_int, _f32p]
lib.sdrhip_debug_record_copied_calls.argtypes = []
lib.sdrhip_debug_record_copied_calls.restype = C.c_longlong
# ---- measurement utilities (include/sdr_hip_bench.h): libsdr_hip_bench.so, a library of its own beside the product (round 6); bench.py and
# tools/ reach them as lib.sdrhip_bench_* like everything else, so the names are attached to `lib` here
BENCH_LIB_PATH = os.path.join(HERE, "lib", "libsdr_hip_bench.so")
if not os.path.exists(BENCH_LIB_PATH):
    raise SdrHipError(f"{BENCH_LIB_PATH} not found: build it with `python -m sdr_amd.build`")
benchlib = C.CDLL(BENCH_LIB_PATH)
for _n in ("sdrhip_bench_stream_8to1", "sdrhip_bench_copy", "sdrhip_bench_copy2", "sdrhip_bench_fm_stream", "sdrhip_bench_fm_stream_latency",
           "sdrhip_bench_pipe", "sdrhip_bench_fm_pipes"):
    setattr(lib, _n, getattr(benchlib, _n))
lib.sdrhip_bench_stream_8to1.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int]
lib.sdrhip_bench_copy.argtypes = [_vp, _vp, _vp, C.c_size_t]
lib.sdrhip_bench_copy2.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int]
lib.sdrhip_bench_fm_stream.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
lib.sdrhip_bench_fm_stream_latency.argtypes = [_vp, C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_double)]
lib.sdrhip_bench_pipe.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
lib.sdrhip_bench_fm_pipes.argtypes = [_vp, _vp, _vp, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
lib.sdrhip_debug_tiled_launches.argtypes = []
lib.sdrhip_debug_tiled_launches.restype = C.c_longlong
lib.sdrhip_dc_blocker_workspace_bytes.argtypes = [C.c_int64]
lib.sdrhip_dc_blocker_workspace_bytes.restype = C.c_size_t
lib.sdrhip_dc_blocker_run.argtypes = [_vp, _vp, _vp, C.c_int64, C.c_float, C.c_float, _vp, _vp, C.c_size_t, C.c_int]
lib.sdrhip_debug_dc_plan.argtypes = [C.c_int64, C.c_int, C.POINTER(_i64), C.POINTER(_i64)]
lib.sdrhip_agc_workspace_bytes.argtypes = [C.c_int64]
lib.sdrhip_agc_workspace_bytes.restype = C.c_size_t
lib.sdrhip_agc_run.argtypes = [_vp, _vp, _vp, C.c_int64, C.c_float, C.c_float, C.c_float, _vp, _vp, C.c_size_t, C.c_int]
lib.sdrhip_debug_agc_plan.argtypes = [C.c_int64, C.c_float, C.c_int, C.POINTER(_i64), C.POINTER(_i64)]
lib.sdrhip_agc_rows_workspace_bytes.argtypes = [C.c_int, C.c_int64]
lib.sdrhip_agc_rows_workspace_bytes.restype = C.c_size_t
lib.sdrhip_agc_run_rows.argtypes = [_vp, _vp, _i64, _vp, _i64, C.c_int, _i64, C.c_float, C.c_float, _vp, _vp, _vp, C.c_size_t, C.c_int]
lib.sdrhip_debug_agc_rows_plan.argtypes = [C.c_int, C.c_int64, C.c_float, C.c_int, C.POINTER(_i64), C.POINTER(_i64)]
lib.sdrhip_dc_blocker_rows_workspace_bytes.argtypes = [C.c_int, C.c_int64]
lib.sdrhip_dc_blocker_rows_workspace_bytes.restype = C.c_size_t
lib.sdrhip_dc_blocker_run_rows.argtypes = [_vp, _vp, _i64, _vp, _i64, C.c_int, _i64, _vp, _vp, _vp, C.c_size_t, C.c_int]
lib.sdrhip_debug_dc_rows_plan.argtypes = [C.c_int, C.c_int64, C.c_int, C.POINTER(_i64), C.POINTER(_i64)]
lib.sdrhip_fm_demod_run_rows.argtypes = [_vp, _vp, _i64, _i64, _vp, _i64, C.c_int, _i64, _i64, _vp, _vp]
lib.sdrhip_deemph_alpha.argtypes = [C.c_double, C.c_double]
lib.sdrhip_deemph_alpha.restype = C.c_float
lib.sdrhip_deemph_workspace_bytes.argtypes = [C.c_int64]
lib.sdrhip_deemph_workspace_bytes.restype = C.c_size_t
lib.sdrhip_deemph_run.argtypes = [_vp, _vp, _vp, C.c_int64, C.c_float, C.c_float, _vp, _vp, C.c_size_t, C.c_int]
lib.sdrhip_deemph_rows_workspace_bytes.argtypes = [C.c_int, C.c_int64]
lib.sdrhip_deemph_rows_workspace_bytes.restype = C.c_size_t
lib.sdrhip_deemph_run_rows.argtypes = [_vp, _vp, _i64, _vp, _i64, C.c_int, _i64, C.c_float, _vp, _vp, _vp, C.c_size_t, C.c_int]
lib.sdrhip_debug_deemph_plan.argtypes = [C.c_int, C.c_int64, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(_i64), C.POINTER(_i64)]
lib.sdrhip_debug_set_deemph_route.argtypes = [C.c_int]
lib.sdrhip_debug_set_deemph_route.restype = None
lib.sdrhip_debug_deemph_launches.argtypes = []
lib.sdrhip_debug_deemph_launches.restype = C.c_longlong
lib.sdrhip_squelch_rows_workspace_bytes.argtypes = [C.c_int, C.c_int64]
lib.sdrhip_squelch_rows_workspace_bytes.restype = C.c_size_t
lib.sdrhip_squelch_run_rows.argtypes = [_vp, _vp, _i64, C.c_int, C.c_int, _vp, _i64, _vp, _i64, C.c_int, C.c_int, _i64, C.c_float, C.c_float,
                                        C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_size_t]
lib.sdrhip_squelch_run.argtypes = [_vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_int, _i64, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int32,
                                   C.c_int32, _vp, _vp, _vp, _vp, C.c_size_t]
lib.sdrhip_debug_squelch_plan.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
lib.sdrhip_debug_set_squelch_route.argtypes = [C.c_int]
lib.sdrhip_debug_set_squelch_route.restype = None
lib.sdrhip_debug_squelch_launches.argtypes = []
lib.sdrhip_debug_squelch_launches.restype = C.c_longlong
lib.sdrhip_am_demod_run.argtypes = [_vp, _vp, _vp, _i64]
lib.sdrhip_am_demod_run_rows.argtypes = [_vp, _vp, _i64, _vp, _i64, C.c_int, _i64]
lib.sdrhip_debug_am_demod_launches.argtypes = []
lib.sdrhip_debug_am_demod_launches.restype = C.c_longlong
lib.sdrhip_debug_rows_launches.argtypes = []
lib.sdrhip_debug_rows_launches.restype = C.c_longlong
lib.sdrhip_filter_run_rows.argtypes = [_vp, _vp, _vp, _i64, _i64, _vp, _i64, C.c_int, _i64, _i64, _i64, C.c_int]
lib.sdrhip_decimator_run_rows.argtypes = [_vp, _vp, _vp, _i64, _i64, _vp, _i64, C.c_int, _i64, _i64, _i64, C.c_int]
lib.sdrhip_resampler_run_rows.argtypes = [_vp, _vp, _vp, _i64, _i64, _vp, _i64, C.c_int, _i64, _i64, _i64, _i64, C.c_int]
lib.sdrhip_debug_fir_rows_plan.argtypes = [_vp, C.c_int, C.c_int, _i64, _i64, _i64, C.POINTER(C.c_int)]
lib.sdrhip_debug_fir_rows_launches.argtypes = []
lib.sdrhip_debug_fir_rows_launches.restype = C.c_longlong
lib.sdrhip_debug_fir_rows_fixups.argtypes = []
lib.sdrhip_debug_fir_rows_fixups.restype = C.c_longlong
lib.sdrhip_audio_tail_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, _f32p, C.c_int, _f32p, C.c_int, C.c_float, _i64]
lib.sdrhip_audio_tail_destroy.argtypes = [_vp]
lib.sdrhip_audio_tail_destroy.restype = None
for _n in ("ready", "first_input"):
    getattr(lib, "sdrhip_audio_tail_" + _n).argtypes = [_vp, _i64]
    getattr(lib, "sdrhip_audio_tail_" + _n).restype = _i64
for _n in ("max_halo", "block"):
    getattr(lib, "sdrhip_audio_tail_" + _n).argtypes = [_vp]
    getattr(lib, "sdrhip_audio_tail_" + _n).restype = _i64
lib.sdrhip_audio_tail_fused_fits.argtypes = [_vp]
lib.sdrhip_audio_tail_shape.argtypes = [_vp, C.POINTER(C.c_int32)]
lib.sdrhip_audio_tail_workspace_bytes.argtypes = [_vp, C.c_int, _i64]
lib.sdrhip_audio_tail_workspace_bytes.restype = C.c_size_t
lib.sdrhip_audio_tail_set_route.argtypes = [_vp, C.c_int]
lib.sdrhip_audio_tail_run_rows.argtypes = [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, C.c_int, _i64, _i64, _vp, C.c_size_t]
lib.sdrhip_debug_audio_tail_launches.argtypes = []
lib.sdrhip_debug_audio_tail_launches.restype = C.c_longlong
lib.sdrhip_audio_tail_general_fits.argtypes = [_vp]
lib.sdrhip_audio_tail_set_general.argtypes = [_vp, C.c_int]
lib.sdrhip_debug_audio_tail_general_launches.argtypes = []
lib.sdrhip_debug_audio_tail_general_launches.restype = C.c_longlong

lib.sdrhip_fm_stream_create.argtypes = [C.POINTER(_vp), _vp, C.c_int, C.c_int]
lib.sdrhip_fm_stream_destroy.argtypes = [_vp]
lib.sdrhip_fm_stream_destroy.restype = None
lib.sdrhip_fm_stream_push.argtypes = [_vp, _u8p, C.c_int]
lib.sdrhip_fm_stream_flush.argtypes = [_vp]
lib.sdrhip_fm_stream_poll.argtypes = [_vp]
lib.sdrhip_fm_stream_set_coalesce.argtypes = [_vp, C.c_int]
lib.sdrhip_fm_stream_set_adaptive.argtypes = [_vp, C.c_int]
lib.sdrhip_fm_stream_input_buffer.argtypes = [_vp]
lib.sdrhip_fm_stream_input_buffer.restype = _vp
lib.sdrhip_fm_stream_pop.argtypes = [_vp, _f32p, C.c_int]
lib.sdrhip_fm_stream_create_bank.argtypes = [C.POINTER(_vp), _vp, C.c_int, C.c_int]
lib.sdrhip_fm_stream_create_bank_i16.argtypes = [C.POINTER(_vp), _vp, C.c_int, C.c_int]
lib.sdrhip_fm_stream_push_i16.argtypes = [_vp, _vp, C.c_int]
lib.sdrhip_fm_stream_input_buffer_i16.argtypes = [_vp]
lib.sdrhip_fm_stream_input_buffer_i16.restype = _vp
lib.sdrhip_fm_stream_rows.argtypes = [_vp]
lib.sdrhip_fm_stream_pop_rows.argtypes = [_vp, _f32p, C.c_int64, C.c_int]

lib.sdrhip_pipe_fir_filter.argtypes = [C.POINTER(_vp), _vp, C.c_int]
lib.sdrhip_pipe_fir_decimator.argtypes = [C.POINTER(_vp), _vp, C.c_int]
lib.sdrhip_pipe_fir_resampler.argtypes = [C.POINTER(_vp), _vp, C.c_int]
lib.sdrhip_pipe_fm_demod.argtypes = [C.POINTER(_vp)]
lib.sdrhip_pipe_am_demod.argtypes = [C.POINTER(_vp)]
lib.sdrhip_pipe_dc_blocker.argtypes = [C.POINTER(_vp)]
lib.sdrhip_pipe_agc.argtypes = [C.POINTER(_vp), C.c_float, C.c_float]
lib.sdrhip_pipe_deemph.argtypes = [C.POINTER(_vp), C.c_float]
lib.sdrhip_pipe_tuner.argtypes = [C.POINTER(_vp), _vp, C.c_int]
lib.sdrhip_pipe_tuner_bank.argtypes = [C.POINTER(_vp), _vp, C.c_int, C.c_int]
lib.sdrhip_pipe_rows.argtypes = [_vp]
lib.sdrhip_pipe_push_u8.argtypes = [_vp, _u8p, C.c_int]
lib.sdrhip_pipe_input_buffer_u8.argtypes = [_vp, C.c_int]
lib.sdrhip_pipe_input_buffer_u8.restype = _vp
lib.sdrhip_pipe_tuner_bank_i16.argtypes = [C.POINTER(_vp), _vp, C.c_int]
lib.sdrhip_pipe_am_bank.argtypes = [C.POINTER(_vp), _vp, C.c_int, C.c_int]
lib.sdrhip_pipe_nfm_bank.argtypes = [C.POINTER(_vp), _vp, C.c_int, C.c_int]
lib.sdrhip_pipe_am_bank_audio.argtypes = [C.POINTER(_vp), _vp, _vp, C.c_int]
lib.sdrhip_pipe_nfm_bank_audio.argtypes = [C.POINTER(_vp), _vp, _vp, C.c_int]
lib.sdrhip_pipe_narrow_bank.argtypes = [C.POINTER(_vp), _vp, C.c_int, C.c_int, C.c_int]
lib.sdrhip_pipe_narrow_bank_audio.argtypes = [C.POINTER(_vp), _vp, _vp, C.c_int, C.c_int]
lib.sdrhip_pipe_push_i16.argtypes = [_vp, _i16p, C.c_int]
lib.sdrhip_pipe_input_buffer_i16.argtypes = [_vp, C.c_int]
lib.sdrhip_pipe_input_buffer_i16.restype = _vp
lib.sdrhip_pipe_pop_rows.argtypes = [_vp, _f32p, _i64, C.c_int]
lib.sdrhip_pipe_spectrum.argtypes = [C.POINTER(_vp), _vp, _i64, C.c_int, C.c_int, C.c_int, C.c_double]
lib.sdrhip_pipe_set_coalesce.argtypes = [_vp, C.c_int]
lib.sdrhip_pipe_set_adaptive.argtypes = [_vp, C.c_int]
lib.sdrhip_pipe_input_buffer.argtypes = [_vp, C.c_int]
lib.sdrhip_pipe_input_buffer.restype = _vp
lib.sdrhip_pipe_push.argtypes = [_vp, _f32p, C.c_int]
lib.sdrhip_pipe_flush.argtypes = [_vp]
lib.sdrhip_pipe_poll.argtypes = [_vp]
lib.sdrhip_pipe_pop.argtypes = [_vp, _f32p, C.c_int]
lib.sdrhip_pipe_destroy.argtypes = [_vp]
lib.sdrhip_pipe_destroy.restype = None

lib.scale.argtypes = [C.c_int, C.c_float, _f32p, _f32p]
lib.scaleSSE.argtypes = [C.c_int, C.c_float, _f32p, _f32p]
lib.scaleAVX.argtypes = [C.c_int, C.c_float, _f32p, _f32p]
lib.fmDemodF.argtypes = [C.c_int, C.c_float, C.c_float, _f32p, _f32p]
lib.dcBlocker.argtypes = [C.c_int, C.c_float, C.c_float, _f32p, _f32p, _f32p, _f32p]
for _n in ("resample2RR", "resampleSSERR", "resampleAVXRR", "resample2RC", "resampleSSERC", "resampleAVXRC"):
    getattr(lib, _n).restype = C.c_int


def check(rc, what="sdrhip call"):
    if rc < 0:
        raise SdrHipError(f"{what} failed ({rc}): {lib.sdrhip_last_error().decode()}")
    return rc


def set_small_launch_outputs(outputs):
    """sdrhip_set_small_launch_outputs: returns the previous threshold."""
    return lib.sdrhip_set_small_launch_outputs(int(outputs))


def version():
    return lib.sdrhip_version().decode()


def device_count():
    return lib.sdrhip_device_count()


def device_name():
    buf = C.create_string_buffer(256)
    check(lib.sdrhip_device_name(buf, 256), "sdrhip_device_name")
    return buf.value.decode()


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a):
    return a.ctypes.data_as(_f32p)


# ---- drop-in symbols on numpy host arrays (what the Haskell FFI would call) ----------
class DropIn:
    """Calls the reference-named symbols exactly as FilterInternal.hs's wrappers do."""

    @staticmethod
    def convert(sym, u8):
        u8 = np.ascontiguousarray(u8, dtype=np.uint8)
        out = np.empty(u8.size, np.float32)
        getattr(lib, sym)(C.c_int(u8.size), u8.ctypes.data_as(_u8p), _fp(out))
        return out

    @staticmethod
    def convert_i16(sym, i16):
        i16 = np.ascontiguousarray(i16, dtype=np.int16)
        out = np.empty(i16.size, np.float32)
        getattr(lib, sym)(C.c_int(i16.size), i16.ctypes.data_as(_i16p), _fp(out))
        return out

    @staticmethod
    def convert_tx(x):
        x = _f32(x)
        out = np.empty(x.size, np.int16)
        lib.convertBladeRFTransmit(C.c_int(x.size), _fp(x), out.ctypes.data_as(_i16p))
        return out

    @staticmethod
    def scale(sym, factor, x):
        x = _f32(x)
        out = np.empty_like(x)
        getattr(lib, sym)(x.size, C.c_float(factor), _fp(x), _fp(out))
        return out

    @staticmethod
    def filt(sym, num, coeffs_as_passed, x, complex_=False):
        c, x = _f32(coeffs_as_passed), _f32(x)
        out = np.empty(num * (2 if complex_ else 1), np.float32)
        getattr(lib, sym)(C.c_int(num), C.c_int(c.size), _fp(c), _fp(x), _fp(out))
        return out

    @staticmethod
    def decim(sym, num, factor, coeffs_as_passed, x, complex_=False):
        c, x = _f32(coeffs_as_passed), _f32(x)
        out = np.empty(num * (2 if complex_ else 1), np.float32)
        getattr(lib, sym)(C.c_int(num), C.c_int(factor), C.c_int(c.size), _fp(c), _fp(x), _fp(out))
        return out

    @staticmethod
    def resample(sym, buf_size, num_coeffs, starting_group, increments, groups, x, complex_=False):
        x = _f32(x)
        out = np.empty(buf_size * (2 if complex_ else 1), np.float32)
        rows = [np.ascontiguousarray(g, dtype=np.float32) for g in groups]
        arr = (_f32p * len(rows))(*[_fp(r) for r in rows])
        inc = np.ascontiguousarray(increments, np.int32)
        g = getattr(lib, sym)(C.c_int(buf_size), C.c_int(num_coeffs), C.c_int(starting_group), C.c_int(len(rows)),
                              inc.ctypes.data_as(_i32p), arr, _fp(x), _fp(out))
        return out, g

    @staticmethod
    def resample_legacy(buf_size, interp, decim, filter_offset, coeffs, x):
        coeffs, x = _f32(coeffs), _f32(x)
        out = np.empty(buf_size, np.float32)
        lib.resampleRR(C.c_int(buf_size), C.c_int(coeffs.size), C.c_int(interp), C.c_int(decim),
                       C.c_int(filter_offset), _fp(coeffs), _fp(x), _fp(out))
        return out

    @staticmethod
    def fm_demod(x_iq, last=(0.0, 0.0)):
        x = _f32(x_iq)
        n = x.size // 2
        out = np.empty(n, np.float32)
        lib.fmDemodF(n, C.c_float(last[0]), C.c_float(last[1]), _fp(x), _fp(out))
        return out

    @staticmethod
    def dc_blocker(x, last_sample=0.0, last_output=0.0):
        x = _f32(x)
        out = np.empty_like(x)
        fs, fo = C.c_float(), C.c_float()
        lib.dcBlocker(x.size, C.c_float(last_sample), C.c_float(last_output), C.byref(fs), C.byref(fo), _fp(x), _fp(out))
        return out, fs.value, fo.value


def dc_plan(n, run_in=0):
    """sdrhip_debug_dc_plan: (chunks, chunk length, run-in) of a dcBlocker run over n samples; chunks == 0: the sequential walk."""
    c, w = _i64(), _i64()
    chunks = check(lib.sdrhip_debug_dc_plan(n, run_in, C.byref(c), C.byref(w)), "sdrhip_debug_dc_plan")
    return chunks, c.value, w.value


def dc_stats(ws):
    """The four statistics words at the start of a dcBlocker / agc workspace (a device tensor of bytes): (chunks left to the
    settle walk, samples it rewrote, chunks recomputed in the repair rounds, chunks speculated on -- 0 = the sequential walk)."""
    return tuple(int(v) for v in ws[:16].cpu().numpy().view(np.uint32))


def agc_plan(n, mu, run_in=0):
    """sdrhip_debug_agc_plan: (chunks, chunk length, run-in) of an agc run over n samples; chunks == 0: the sequential walk."""
    c, w = _i64(), _i64()
    chunks = check(lib.sdrhip_debug_agc_plan(n, mu, run_in, C.byref(c), C.byref(w)), "sdrhip_debug_agc_plan")
    return chunks, c.value, w.value


def agc(x, mu, reference, state=1.0, run_in=0):
    """agc (Util.hs:325-342) -> (out, final_state).  x: a device tensor (complex64, or float32 interleaved; `out` is then a
    device tensor of the same type and shape) or a host array (complex64 or float32 interleaved; `out` is a numpy array)."""
    if hasattr(x, "data_ptr"):
        import torch
        n = x.numel() if x.is_complex() else x.numel() // 2
        d_in = x.contiguous()
        d_out = torch.empty_like(d_in)
        fin = torch.empty(1, dtype=torch.float32, device=d_in.device)
        wsb = lib.sdrhip_agc_workspace_bytes(n)
        ws = torch.empty(wsb, dtype=torch.uint8, device=d_in.device)
        check(lib.sdrhip_agc_run(torch.cuda.current_stream().cuda_stream, d_in.data_ptr(), d_out.data_ptr(), n, mu, reference, state,
                                 fin.data_ptr(), ws.data_ptr(), wsb, run_in), "sdrhip_agc_run")
        return d_out, float(fin.item())
    a = np.ascontiguousarray(x)
    cplx = np.iscomplexobj(a)
    a = np.ascontiguousarray(a, dtype=np.complex64 if cplx else np.float32)
    n = a.size if cplx else a.size // 2
    out = np.empty_like(a)
    fin = np.empty(1, np.float32)
    wsb = lib.sdrhip_agc_workspace_bytes(n)
    bufs = [_vp(), _vp(), _vp(), _vp()]
    try:
        for b, size in zip(bufs, (max(8 * n, 8), max(8 * n, 8), 4, wsb)):
            check(lib.sdrhip_malloc(C.byref(b), size), "sdrhip_malloc")
        d_in, d_out, d_fin, d_ws = bufs
        check(lib.sdrhip_memcpy_h2d(d_in, a.ctypes.data, 8 * n, None), "sdrhip_memcpy_h2d")
        check(lib.sdrhip_agc_run(None, d_in, d_out, n, mu, reference, state, d_fin, d_ws, wsb, run_in), "sdrhip_agc_run")
        check(lib.sdrhip_memcpy_d2h(out.ctypes.data, d_out, 8 * n, None), "sdrhip_memcpy_d2h")
        check(lib.sdrhip_memcpy_d2h(fin.ctypes.data, d_fin, 4, None), "sdrhip_memcpy_d2h")
        check(lib.sdrhip_stream_sync(None), "sdrhip_stream_sync")
    finally:
        for b in bufs:
            if b:
                lib.sdrhip_free(b)
    return out, float(fin[0])


# ---- row forms: every row of a bank in one launch set ---------------------------------------------------------------------------
ROWS_MAX = 1024


def agc_rows_plan(rows, n, mu, run_in=0):
    """sdrhip_debug_agc_rows_plan: (chunks per row, chunk length, run-in); rows == 1 gives agc_plan(n, mu, run_in)."""
    c, w = _i64(), _i64()
    chunks = check(lib.sdrhip_debug_agc_rows_plan(rows, n, mu, run_in, C.byref(c), C.byref(w)), "sdrhip_debug_agc_rows_plan")
    return chunks, c.value, w.value


def dc_rows_plan(rows, n, run_in=0):
    """sdrhip_debug_dc_rows_plan: (chunks per row, chunk length, run-in); rows == 1 gives dc_plan(n, run_in)."""
    c, w = _i64(), _i64()
    chunks = check(lib.sdrhip_debug_dc_rows_plan(rows, n, run_in, C.byref(c), C.byref(w)), "sdrhip_debug_dc_rows_plan")
    return chunks, c.value, w.value


def rows_stats(ws, rows):
    """The statistics words at the start of a rows workspace (a device tensor of bytes): per row the four words of dc_stats."""
    w = ws[:16 * rows].cpu().numpy().view(np.uint32).reshape(rows, 4)
    return [tuple(int(v) for v in r) for r in w]


def rows_launches():
    """sdrhip_debug_rows_launches: kernel launches of the row forms in this process."""
    return int(lib.sdrhip_debug_rows_launches())


def _rows_of(t, what, floats_per_sample=1):
    """(rows, samples per row, row stride in floats) of a 2-D device tensor whose rows are contiguous: complex64 (a sample is one
    element) or float32 (a sample is floats_per_sample floats).  The stride may be anything: a view into a bank's output works."""
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{what}: a 2-D tensor with contiguous rows is needed")
    if t.is_complex():
        return t.shape[0], t.shape[1], 2 * t.stride(0)
    if t.shape[1] % floats_per_sample:
        raise ValueError(f"{what}: {t.shape[1]} floats per row is not a whole number of samples")
    return t.shape[0], t.shape[1] // floats_per_sample, t.stride(0)


def _dptr(t):
    """data_ptr(), also for a view without elements (torch reports 0 there, and the library refuses null pointers)"""
    return t.data_ptr() if t.numel() else t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size()


def _rows_empty(rows, width, dtype, device):
    import torch
    return torch.empty(max(rows * width, 1), dtype=dtype, device=device)[:rows * width].view(rows, width)


def _rows_workspace(workspace, nbytes, device):
    """workspace: "auto" = allocate; None = none (every row takes the sequential walk); or a device tensor of bytes."""
    import torch
    if workspace is None:
        return None, 0, 0
    if isinstance(workspace, str):
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return workspace, workspace.data_ptr(), workspace.numel()


def agc_rows(x, mu, reference, states, run_in=0, out=None, final=None, workspace="auto"):
    """sdrhip_agc_run_rows on the current stream -> (out, final).  x: rows x n complex64, or rows x 2n float32 interleaved, on the
    device, rows contiguous, any row stride (a view will do).  states: rows float32 on the device.  out (default: a new
    contiguous tensor like x) and final (default: new; may be `states`) as given.  No synchronisation."""
    import torch
    rows, n, in_stride = _rows_of(x, "agc_rows", 2)
    if out is None:
        out = _rows_empty(rows, x.shape[1], x.dtype, x.device)
    orows, on, out_stride = _rows_of(out, "agc_rows", 2)
    if (orows, on) != (rows, n) or states.numel() != rows or states.dtype != torch.float32:
        raise ValueError("agc_rows: out and states must match x's rows")
    if final is None:
        final = torch.empty(rows, dtype=torch.float32, device=x.device)
    ws, ws_ptr, ws_bytes = _rows_workspace(workspace, lib.sdrhip_agc_rows_workspace_bytes(rows, n), x.device)
    check(lib.sdrhip_agc_run_rows(torch.cuda.current_stream().cuda_stream, _dptr(x), in_stride, _dptr(out), out_stride, rows, n,
                                  mu, reference, states.data_ptr(), final.data_ptr(), ws_ptr, ws_bytes, run_in), "sdrhip_agc_run_rows")
    return out, final


def dc_blocker_rows(x, states, run_in=0, out=None, final=None, workspace="auto"):
    """sdrhip_dc_blocker_run_rows on the current stream -> (out, final).  x: rows x n float32 on the device, rows contiguous, any
    row stride.  states: rows x 2 float32 (last_sample, last_output) on the device; final likewise (default: new; may be `states`)."""
    import torch
    rows, n, in_stride = _rows_of(x, "dc_blocker_rows")
    if out is None:
        out = _rows_empty(rows, n, torch.float32, x.device)
    orows, on, out_stride = _rows_of(out, "dc_blocker_rows")
    if (orows, on) != (rows, n) or states.numel() != 2 * rows or states.dtype != torch.float32 or not states.is_contiguous():
        raise ValueError("dc_blocker_rows: out and states must match x's rows")
    if final is None:
        final = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    ws, ws_ptr, ws_bytes = _rows_workspace(workspace, lib.sdrhip_dc_blocker_rows_workspace_bytes(rows, n), x.device)
    check(lib.sdrhip_dc_blocker_run_rows(torch.cuda.current_stream().cuda_stream, _dptr(x), in_stride, _dptr(out), out_stride,
                                         rows, n, states.data_ptr(), final.data_ptr(), ws_ptr, ws_bytes, run_in),
          "sdrhip_dc_blocker_run_rows")
    return out, final


# ---- de-emphasis (sdr_hip.h "de-emphasis") ---------------------------------------------------------------------------------------
DEEMPH_AUTO, DEEMPH_SEQ, DEEMPH_WG, DEEMPH_LS = 0, 1, 2, 3


def deemph_alpha(tau_seconds, sample_rate):
    """sdrhip_deemph_alpha: float32(1 - exp(-1 / (tau * rate))) as a Python float; 0.0 for arguments that are not finite and positive."""
    return float(lib.sdrhip_deemph_alpha(tau_seconds, sample_rate))


def deemph_plan(rows, n, alpha, run_in=0, has_workspace=True):
    """sdrhip_debug_deemph_plan: (chunks per row, route, chunk length, run-in); route 1 SEQ (chunks == 0), 2 WG, 3 LS."""
    r, c, w = C.c_int(), _i64(), _i64()
    chunks = check(lib.sdrhip_debug_deemph_plan(rows, n, alpha, run_in, int(bool(has_workspace)), C.byref(r), C.byref(c), C.byref(w)),
                   "sdrhip_debug_deemph_plan")
    return chunks, r.value, c.value, w.value


def set_deemph_route(route):
    """sdrhip_debug_set_deemph_route: 0 auto, 1 SEQ, 2 WG, 3 LS, process-wide; a forced route that does not fit a call is refused."""
    lib.sdrhip_debug_set_deemph_route(int(route))


def deemph_launches():
    """sdrhip_debug_deemph_launches: kernel launches of the de-emphasis calls in this process (1 per SEQ or WG call, 5 per LS call)."""
    return int(lib.sdrhip_debug_deemph_launches())


def deemph_rows(x, alpha, states, run_in=0, out=None, final=None, workspace="auto"):
    """sdrhip_deemph_run_rows on the current stream -> (out, final).  x: rows x n float32 on the device, rows contiguous, any row
    stride (a view into a bank's audio will do).  states: rows float32 on the device; final likewise (default: new; may be `states`).
    workspace: "auto" = allocate, None = none, or a device tensor of bytes.  No synchronisation."""
    import torch
    rows, n, in_stride = _rows_of(x, "deemph_rows")
    if out is None:
        out = _rows_empty(rows, n, torch.float32, x.device)
    orows, on, out_stride = _rows_of(out, "deemph_rows")
    if (orows, on) != (rows, n) or states.numel() != rows or states.dtype != torch.float32 or not states.is_contiguous():
        raise ValueError("deemph_rows: out and states must match x's rows")
    if final is None:
        final = torch.empty(rows, dtype=torch.float32, device=x.device)
    ws, ws_ptr, ws_bytes = _rows_workspace(workspace, lib.sdrhip_deemph_rows_workspace_bytes(rows, n), x.device)
    check(lib.sdrhip_deemph_run_rows(torch.cuda.current_stream().cuda_stream, _dptr(x), in_stride, _dptr(out), out_stride, rows, n,
                                     alpha, states.data_ptr(), final.data_ptr(), ws_ptr or None, ws_bytes, run_in), "sdrhip_deemph_run_rows")
    return out, final


def deemph(x, alpha, state=0.0, run_in=0):
    """sdrhip_deemph_run on the current stream -> (out, final): x a 1-D float32 device tensor, final a device tensor of one float.
    No synchronisation."""
    import torch
    x = x.contiguous()
    n = x.numel()
    out = torch.empty(max(n, 1), dtype=torch.float32, device=x.device)[:n]
    final = torch.empty(1, dtype=torch.float32, device=x.device)
    wsb = lib.sdrhip_deemph_workspace_bytes(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    check(lib.sdrhip_deemph_run(torch.cuda.current_stream().cuda_stream, _dptr(x), _dptr(out), n, alpha, state, final.data_ptr(),
                                ws.data_ptr(), wsb, run_in), "sdrhip_deemph_run")
    return out, final


# ---- squelch (sdr_hip.h "squelch") -----------------------------------------------------------------------------------------------
SQUELCH_AUTO, SQUELCH_WG, SQUELCH_LS = 0, 1, 2


def squelch_plan(rows, n_blocks, block_det, det_complex=False, block_sig=0, has_workspace=True):
    """sdrhip_debug_squelch_plan: (kernel launches, route); route 1 WG, 2 LS; block_sig = 0 is detect-only."""
    r = C.c_int()
    launches = check(lib.sdrhip_debug_squelch_plan(rows, n_blocks, block_det, int(bool(det_complex)), block_sig, int(bool(has_workspace)),
                                                   C.byref(r)), "sdrhip_debug_squelch_plan")
    return launches, r.value


def set_squelch_route(route):
    """sdrhip_debug_set_squelch_route: 0 auto, 1 WG, 2 LS, process-wide; forced LS without a workspace is refused."""
    lib.sdrhip_debug_set_squelch_route(int(route))


def squelch_launches():
    """sdrhip_debug_squelch_launches: kernel launches of the squelch calls in this process."""
    return int(lib.sdrhip_debug_squelch_launches())


def squelch_run_rows(det, block_det, sig, block_sig, open_level, close_level, hang_blocks=0, open_above=True, states=None, out=None,
                     final=None, levels=None, gates=None, workspace="auto", n_blocks=None):
    """sdrhip_squelch_run_rows on the current stream -> (out, final, levels, gates).  det: rows x m complex64 (a complex detector) or
    rows x m float32 (a real one) on the device, rows contiguous, any row stride.  sig: rows x (n_blocks * block_sig) float32, `det`
    itself for self-detection, or None for detect-only (out is None then).  out: default a new tensor; `sig` gates in place.
    states: rows x 2 int32 on the device or None ({0, 0}); final likewise (default: new; may be `states`).  levels / gates: True for
    new tensors, a tensor to fill, or None.  n_blocks defaults to the whole blocks of det.  No synchronisation."""
    import torch
    cplx = det.is_complex()
    rows, m, det_stride = _rows_of(det, "squelch_run_rows")
    if n_blocks is None:
        n_blocks = m // block_det
    in_stride = out_stride = 0
    if sig is not None:
        srows, sn, in_stride = _rows_of(sig, "squelch_run_rows")
        if srows != rows or sn < n_blocks * block_sig or sig.dtype != torch.float32:
            raise ValueError("squelch_run_rows: sig must be float32 with det's rows and n_blocks * block_sig floats in each")
        if out is None:
            out = _rows_empty(rows, n_blocks * block_sig, torch.float32, sig.device)
        orows, on, out_stride = _rows_of(out, "squelch_run_rows")
        if orows != rows or on < n_blocks * block_sig:
            raise ValueError("squelch_run_rows: out must match sig")
    if states is not None and (states.numel() != 2 * rows or states.dtype != torch.int32 or not states.is_contiguous()):
        raise ValueError("squelch_run_rows: states must be rows x 2 int32")
    if final is None:
        final = torch.empty((rows, 2), dtype=torch.int32, device=det.device)
    if levels is True:
        levels = _rows_empty(rows, n_blocks, torch.float32, det.device)
    if gates is True:
        gates = _rows_empty(rows, n_blocks, torch.uint8, det.device)
    ws, ws_ptr, ws_bytes = _rows_workspace(workspace, lib.sdrhip_squelch_rows_workspace_bytes(rows, n_blocks), det.device)
    check(lib.sdrhip_squelch_run_rows(torch.cuda.current_stream().cuda_stream, _dptr(det), det_stride, int(cplx), block_det,
                                      _dptr(sig) if sig is not None else None, in_stride, _dptr(out) if sig is not None else None,
                                      out_stride, block_sig, rows, n_blocks, open_level, close_level, hang_blocks, int(bool(open_above)),
                                      states.data_ptr() if states is not None else None, final.data_ptr(),
                                      _dptr(levels) if levels is not None else None, _dptr(gates) if gates is not None else None,
                                      ws_ptr or None, ws_bytes), "sdrhip_squelch_run_rows")
    return (out if sig is not None else None), final, levels, gates


def squelch_run(det, block_det, sig, block_sig, open_level, close_level, hang_blocks=0, open_above=True, state=(0, 0), levels=None,
                gates=None):
    """sdrhip_squelch_run on the current stream -> (out, final, levels, gates): det a 1-D complex64 or float32 device tensor, sig a
    1-D float32 device tensor (`det` itself for self-detection) or None for detect-only; final a device tensor of two int32."""
    import torch
    cplx = det.is_complex()
    n_blocks = det.numel() // block_det
    out = None
    if sig is not None:
        out = torch.empty(max(n_blocks * block_sig, 1), dtype=torch.float32, device=det.device)[:n_blocks * block_sig]
    final = torch.empty(2, dtype=torch.int32, device=det.device)
    if levels is True:
        levels = torch.empty(max(n_blocks, 1), dtype=torch.float32, device=det.device)[:n_blocks]
    if gates is True:
        gates = torch.empty(max(n_blocks, 1), dtype=torch.uint8, device=det.device)[:n_blocks]
    wsb = lib.sdrhip_squelch_rows_workspace_bytes(1, n_blocks)
    ws = torch.empty(wsb, dtype=torch.uint8, device=det.device)
    check(lib.sdrhip_squelch_run(torch.cuda.current_stream().cuda_stream, _dptr(det), int(cplx), block_det,
                                 _dptr(sig) if sig is not None else None, _dptr(out) if sig is not None else None, block_sig, n_blocks,
                                 open_level, close_level, hang_blocks, int(bool(open_above)), int(state[0]), int(state[1]), final.data_ptr(),
                                 _dptr(levels) if levels is not None else None, _dptr(gates) if gates is not None else None,
                                 ws.data_ptr(), wsb), "sdrhip_squelch_run")
    return out, final, levels, gates


def fm_demod_rows(x, last=None, out=None, last_out=None, in_base=0, k_begin=None, k_end=None):
    """sdrhip_fm_demod_run_rows on the current stream -> out (rows x (k_end - k_begin) float32).  x: rows x m complex64 or rows x 2m
    float32 interleaved on the device: each row holds its samples in_base .. in_base + m.  k_begin / k_end default to the whole
    row.  last: rows x 2 float32 on the device, the rows' predecessors when k_begin == in_base (None: (0, 0)); last_out, if given
    (it may be `last`), receives each row's sample k_end - 1."""
    import torch
    rows, m, in_stride = _rows_of(x, "fm_demod_rows", 2)
    k_begin = in_base if k_begin is None else k_begin
    k_end = in_base + m if k_end is None else k_end
    if not in_base <= k_begin <= k_end <= in_base + m:
        raise ValueError("fm_demod_rows: [k_begin, k_end) must lie inside the rows")
    if out is None:
        out = _rows_empty(rows, k_end - k_begin, torch.float32, x.device)
    orows, on, out_stride = _rows_of(out, "fm_demod_rows")
    if (orows, on) != (rows, k_end - k_begin) or out.dtype != torch.float32:
        raise ValueError("fm_demod_rows: out must be rows x (k_end - k_begin) float32")
    for t in (last, last_out):
        if t is not None and (t.numel() != 2 * rows or t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError("fm_demod_rows: last / last_out are rows x 2 float32")
    check(lib.sdrhip_fm_demod_run_rows(torch.cuda.current_stream().cuda_stream, _dptr(x), in_stride, in_base, _dptr(out),
                                       out_stride, rows, k_begin, k_end, last.data_ptr() if last is not None else None,
                                       last_out.data_ptr() if last_out is not None else None), "sdrhip_fm_demod_run_rows")
    return out


def am_demod_launches():
    """sdrhip_debug_am_demod_launches: kernel launches of am_demod / am_demod_rows in this process."""
    return int(lib.sdrhip_debug_am_demod_launches())


def am_demod(d_in, n, d_out, stream=None):
    """sdrhip_am_demod_run: n interleaved complex float32 samples at device address d_in -> n float32 at d_out,
    out[i] = Data.Complex.magnitude at Float of sample i (the envelope detector of an AM receiver).  d_in / d_out: device tensors or
    raw device addresses, any 4-byte alignment.  Asynchronous on `stream` (a raw stream handle; None: the null stream)."""
    pin = _dptr(d_in) if hasattr(d_in, "data_ptr") else d_in
    pout = _dptr(d_out) if hasattr(d_out, "data_ptr") else d_out
    check(lib.sdrhip_am_demod_run(stream, pin, pout, n), "sdrhip_am_demod_run")


def am_demod_rows(x, out=None):
    """sdrhip_am_demod_run_rows on the current stream -> out (rows x n float32).  x: rows x n complex64 or rows x 2n float32
    interleaved on the device, rows contiguous, any row stride: a view into a TunerBank output works.  No synchronisation."""
    import torch
    rows, n, in_stride = _rows_of(x, "am_demod_rows", 2)
    if out is None:
        out = _rows_empty(rows, n, torch.float32, x.device)
    orows, on, out_stride = _rows_of(out, "am_demod_rows")
    if (orows, on) != (rows, n) or out.dtype != torch.float32:
        raise ValueError("am_demod_rows: out must be rows x n float32")
    check(lib.sdrhip_am_demod_run_rows(torch.cuda.current_stream().cuda_stream, _dptr(x), in_stride, _dptr(out), out_stride, rows, n),
          "sdrhip_am_demod_run_rows")
    return out


# ---- row forms of the FIR operators --------------------------------------------------------
FIR_ROWS_AUTO, FIR_ROWS_BANKED, FIR_ROWS_ROW_BY_ROW = 0, 1, 2


def fir_rows_launches():
    """sdrhip_debug_fir_rows_launches: banked tile launches of the FIR row forms in this process (fix-ups not counted)."""
    return int(lib.sdrhip_debug_fir_rows_launches())


def fir_rows_fixups():
    """sdrhip_debug_fir_rows_fixups: banked seam fix-up launches of the FIR row forms in this process."""
    return int(lib.sdrhip_debug_fir_rows_fixups())


def fir_rows_plan(desc, k_begin, k_end, rows=1, seam_block=0):
    """sdrhip_debug_fir_rows_plan for a Filter / Decimator / Resampler: None where the banked route does not serve the shape, else a
    dict: cycles_per_tile, tiles_per_row, per_lane (independent outputs per lane), per_cycle (outputs per cycle: a resampler's
    groups), tile_outputs, and split_cycles_per_tile / split_per_lane: what the one-row lane-split kernel plans for one such row."""
    kind = 0 if isinstance(desc, Filter) else 1 if isinstance(desc, Decimator) else 2
    p = (C.c_int * 6)()
    if not check(lib.sdrhip_debug_fir_rows_plan(desc.h, kind, rows, k_begin, k_end, seam_block, p), "sdrhip_debug_fir_rows_plan"):
        return None
    return {"cycles_per_tile": p[0], "tiles_per_row": p[1], "per_lane": p[2], "per_cycle": p[3], "tile_outputs": p[0] * p[3],
            "split_cycles_per_tile": p[4], "split_per_lane": p[5]}


def _fir_rows_side(t, stride, rows, cplx, what):
    """(pointer, stride in floats, rows or None) of one side of a FIR rows call: a 2-D device tensor with contiguous rows (complex64,
    or float32 -- interleaved pairs on a complex operator), any row stride, or a device pointer with the stride given."""
    if isinstance(t, int) or t is None:
        if stride is None:
            raise ValueError(f"{what}: a pointer needs its row stride")
        return t, int(stride), rows
    r, _, st = _rows_of(t, what, 2 if cplx and not t.is_complex() else 1)
    if t.is_complex() != bool(cplx) and t.is_complex():
        raise ValueError(f"{what}: complex rows on a real operator")
    return _dptr(t), st if stride is None else int(stride), r


def _fir_rows_call(fn, name, desc, x, out, k_begin, k_end, in_base, tail, route, stream, in_stride, out_stride, rows):
    px, ist, r_in = _fir_rows_side(x, in_stride, rows, desc.complex, name)
    po, ost, r_out = _fir_rows_side(out, out_stride, rows, desc.complex, name)
    rows = rows if rows is not None else r_in if r_in is not None else r_out
    if rows is None or any(r is not None and r != rows for r in (r_in, r_out)):
        raise ValueError(f"{name}: the two sides must have the same number of rows (pointers: pass rows=)")
    if stream is None and not (isinstance(x, int) and isinstance(out, int)):
        import torch
        stream = torch.cuda.current_stream().cuda_stream
    check(fn(desc.h, stream, px, ist, in_base, po, ost, rows, k_begin, k_end, *tail, route), name)
    return out


# ---- descriptors ----------------------------------------------------------------------
class _Handle:
    _destroy = None

    def __init__(self):
        self.h = _vp()

    def close(self):
        if self.h:
            type(self)._destroy(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Filter(_Handle):
    """fastFilter{C,SSE,AVX}{R,C} / fastFilterSym{SSE,AVX}R (Filter.hs:163-261)."""
    _destroy = lib.sdrhip_filter_destroy

    def __init__(self, coeffs, order=ORDER_AVX, complex_=False, sym=False):
        super().__init__()
        c = _f32(coeffs)
        if sym:
            check(lib.sdrhip_filter_sym_create(C.byref(self.h), order, _fp(c), c.size), "sdrhip_filter_sym_create")
        else:
            check(lib.sdrhip_filter_create(C.byref(self.h), order, int(complex_), _fp(c), c.size), "sdrhip_filter_create")
        self.complex = complex_
        self.num_coeffs = lib.sdrhip_filter_num_coeffs(self.h)

    def run(self, d_in, in_base, d_out, k_begin, k_end, seam_block=0, stream=None):
        check(lib.sdrhip_filter_run(self.h, stream, d_in, in_base, d_out, k_begin, k_end, seam_block), "sdrhip_filter_run")

    def run_rows(self, x, out, k_begin, k_end, in_base=0, seam_block=0, route=FIR_ROWS_AUTO, stream=None, in_stride=None,
                 out_stride=None, rows=None):
        """sdrhip_filter_run_rows: outputs [k_begin, k_end) of every row, row r of x (its stream from element in_base on) -> row r of
        out.  x / out: 2-D device tensors with contiguous rows and any row stride (a view into a bank's output will do), on the
        current stream -- or device pointers with in_stride / out_stride (floats) and rows.  No synchronisation.  -> out"""
        return _fir_rows_call(lib.sdrhip_filter_run_rows, "sdrhip_filter_run_rows", self, x, out, k_begin, k_end, in_base, (seam_block,),
                              route, stream, in_stride, out_stride, rows)


class Decimator(_Handle):
    """fastDecimator{C,SSE,AVX}{R,C} / fastDecimatorSym{SSE,AVX}R (Filter.hs:277-387)."""
    _destroy = lib.sdrhip_decimator_destroy

    def __init__(self, factor, coeffs, order=ORDER_AVX, complex_=False, sym=False):
        super().__init__()
        c = _f32(coeffs)
        if sym:
            check(lib.sdrhip_decimator_sym_create(C.byref(self.h), order, factor, _fp(c), c.size), "sdrhip_decimator_sym_create")
        else:
            check(lib.sdrhip_decimator_create(C.byref(self.h), order, int(complex_), factor, _fp(c), c.size), "sdrhip_decimator_create")
        self.complex = complex_
        self.factor = factor
        self.num_coeffs = lib.sdrhip_decimator_num_coeffs(self.h)

    def run(self, d_in, in_base, d_out, k_begin, k_end, seam_block=0, stream=None):
        check(lib.sdrhip_decimator_run(self.h, stream, d_in, in_base, d_out, k_begin, k_end, seam_block), "sdrhip_decimator_run")

    def run_rows(self, x, out, k_begin, k_end, in_base=0, seam_block=0, route=FIR_ROWS_AUTO, stream=None, in_stride=None,
                 out_stride=None, rows=None):
        """sdrhip_decimator_run_rows: as Filter.run_rows (row r of x holds its inputs from element in_base on)."""
        return _fir_rows_call(lib.sdrhip_decimator_run_rows, "sdrhip_decimator_run_rows", self, x, out, k_begin, k_end, in_base,
                              (seam_block,), route, stream, in_stride, out_stride, rows)

    def run_u8(self, d_in, in_base, d_out, k_begin, k_end, seam_block=0, stream=None):
        check(lib.sdrhip_decimator_run_u8(self.h, stream, d_in, in_base, d_out, k_begin, k_end, seam_block), "sdrhip_decimator_run_u8")


class Resampler(_Handle):
    """fastResampler{C,SSE,AVX}{R,C} (Filter.hs:408-502)."""
    _destroy = lib.sdrhip_resampler_destroy

    def __init__(self, interpolation, decimation, coeffs, order=ORDER_AVX, complex_=False):
        super().__init__()
        c = _f32(coeffs)
        check(lib.sdrhip_resampler_create(C.byref(self.h), order, int(complex_), interpolation, decimation, _fp(c), c.size),
              "sdrhip_resampler_create")
        self.complex = complex_
        self.I, self.D = interpolation, decimation
        self.num_coeffs = lib.sdrhip_resampler_num_coeffs(self.h)
        self.num_groups = lib.sdrhip_resampler_num_groups(self.h)

    def in_offset(self, m):
        return lib.sdrhip_resampler_in_offset(self.h, m)

    def filter_offset(self, m):
        return lib.sdrhip_resampler_filter_offset(self.h, m)

    def group(self, m):
        return lib.sdrhip_resampler_group(self.h, m)

    def run(self, d_in, in_base, d_out, k_begin, k_end, seam_block=0, stream=None, out_block=0):
        check(lib.sdrhip_resampler_run(self.h, stream, d_in, in_base, d_out, k_begin, k_end, seam_block, out_block),
              "sdrhip_resampler_run")

    def run_rows(self, x, out, k_begin, k_end, in_base=0, seam_block=0, out_block=0, route=FIR_ROWS_AUTO, stream=None, in_stride=None,
                 out_stride=None, rows=None):
        """sdrhip_resampler_run_rows: as Filter.run_rows, with the Pipe's output block size as in run()."""
        return _fir_rows_call(lib.sdrhip_resampler_run_rows, "sdrhip_resampler_run_rows", self, x, out, k_begin, k_end, in_base,
                              (seam_block, out_block), route, stream, in_stride, out_stride, rows)


AUDIO_TAIL_AUTO, AUDIO_TAIL_FUSED, AUDIO_TAIL_COMPOSED = 0, 1, 2


def audio_tail_launches():
    """sdrhip_debug_audio_tail_launches: launches of the fused audio-tail kernel in this process."""
    return int(lib.sdrhip_debug_audio_tail_launches())


AUDIO_TAIL_GENERAL_AUTO, AUDIO_TAIL_GENERAL_ALWAYS, AUDIO_TAIL_GENERAL_NEVER = 0, 1, 2


def audio_tail_general_launches():
    """sdrhip_debug_audio_tail_general_launches: launches of the general fused audio-tail kernel in this process."""
    return int(lib.sdrhip_debug_audio_tail_general_launches())


class AudioTail(_Handle):
    """sdrhip_audio_tail: firResampler(block) >-> firFilter(block) >-> (* gain) over rows of real demodulated samples -- the audio
    stages behind AmBank / NfmBank.  Arguments as FmChain's tail; block = the one block size of every Pipe (0 = contiguous).
    ready / first_input / max_halo / workspace_bytes are host arithmetic and need no GPU."""
    _destroy = lib.sdrhip_audio_tail_destroy

    def __init__(self, interpolation, decimation, resamp_taps, audio_half_taps, gain=1.0, block=0, order=ORDER_AVX):
        super().__init__()
        r, a = _f32(resamp_taps), _f32(audio_half_taps)
        check(lib.sdrhip_audio_tail_create(C.byref(self.h), order, interpolation, decimation, _fp(r), r.size, _fp(a), a.size, gain, block),
              "sdrhip_audio_tail_create")
        self.block = block

    def ready(self, n_y):
        return lib.sdrhip_audio_tail_ready(self.h, n_y)

    def first_input(self, q):
        return lib.sdrhip_audio_tail_first_input(self.h, q)

    def max_halo(self):
        return lib.sdrhip_audio_tail_max_halo(self.h)

    def fused_fits(self):
        return bool(check(lib.sdrhip_audio_tail_fused_fits(self.h), "sdrhip_audio_tail_fused_fits"))

    def workspace_bytes(self, rows, n_y):
        return lib.sdrhip_audio_tail_workspace_bytes(self.h, rows, n_y)

    def set_route(self, route):
        """0 = auto, 1 = the fused kernel (one launch, no workspace), 2 = the composition of the row forms (the definition)"""
        check(lib.sdrhip_audio_tail_set_route(self.h, route), "sdrhip_audio_tail_set_route")

    def general_fits(self):
        return bool(check(lib.sdrhip_audio_tail_general_fits(self.h), "sdrhip_audio_tail_general_fits"))

    def set_general(self, mode):
        """route 0 only, behind route 1's rule: 0 = the general fused kernel by its measured rule, 1 = wherever it fits, 2 = never"""
        check(lib.sdrhip_audio_tail_set_general(self.h, mode), "sdrhip_audio_tail_set_general")

    def run_rows(self, y, audio, q0, q1, y_base=0, n_y=None, workspace=None, workspace_bytes=None, stream=None, y_stride=None,
                 audio_stride=None, rows=None):
        """sdrhip_audio_tail_run_rows: audio outputs [q0, q1) of every row; row r of y holds its stream elements [y_base, y_base + n_y).
        y / audio: 2-D float32 device tensors with contiguous rows and any row stride (n_y defaults to y's width), on the current
        stream -- or device pointers with y_stride / audio_stride (floats), rows and n_y.  workspace: a device tensor or a pointer
        with workspace_bytes (routes 0 and 2).  No synchronisation.  -> audio"""
        name = "sdrhip_audio_tail_run_rows"
        py, yst, r_in = _fir_rows_side(y, y_stride, rows, False, name)
        pa, ast, r_out = _fir_rows_side(audio, audio_stride, rows, False, name)
        rows = rows if rows is not None else r_in if r_in is not None else r_out
        if rows is None or any(r is not None and r != rows for r in (r_in, r_out)):
            raise ValueError(f"{name}: the two sides must have the same number of rows (pointers: pass rows=)")
        if n_y is None:
            if isinstance(y, int) or y is None:
                raise ValueError(f"{name}: a pointer needs n_y")
            n_y = y.shape[1]
        if workspace is not None and not isinstance(workspace, int):
            workspace_bytes = workspace.numel() * workspace.element_size() if workspace_bytes is None else workspace_bytes
            workspace = _dptr(workspace)
        if stream is None and not (isinstance(y, int) and isinstance(audio, int)):
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        check(lib.sdrhip_audio_tail_run_rows(self.h, stream, py, yst, y_base, n_y, pa, ast, rows, q0, q1, workspace, workspace_bytes or 0), name)
        return audio


TUNER_ROUTE_AUTO, TUNER_ROUTE_FUSED, TUNER_ROUTE_TWO_PASS = 0, 1, 2


def tuner_shift_table(num, den):
    """sdrhip_tuner_shift_table: exp(2 pi i ((num n) mod den) / den), n < den, as interleaved float32 (re, im) pairs.
    (1, 4) = quarterBandUp, (1, 2) = halfBandUp (Util.hs:263-285).  Host code: no device needed."""
    out = np.empty(2 * int(den), np.float32)
    check(lib.sdrhip_tuner_shift_table(int(num), int(den), _fp(out)), "sdrhip_tuner_shift_table")
    return out


def small_chain_tuned_launches():
    """Launches of the tuned one-kernel chain so far (sdrhip_debug_small_chain_tuned_launches)."""
    return int(lib.sdrhip_debug_small_chain_tuned_launches())


def tuner_fused_launches():
    return int(lib.sdrhip_debug_tuner_fused_launches())


def set_tuner_chunk(samples):
    """sdrhip_debug_set_tuner_chunk (test knob of the two-pass route): returns the previous value."""
    return int(lib.sdrhip_debug_set_tuner_chunk(int(samples)))


class Tuner(_Handle):
    """`P.map (VG.zipWith (*) osc) >-> firDecimator`: a periodic complex oscillator (osc_iq: interleaved float32 pairs, indexed by the
    absolute stream position) mixed into a complex decimator (sdr_hip.h, sdrhip_tuner_*)."""
    _destroy = lib.sdrhip_tuner_destroy
    complex = True

    def __init__(self, factor, coeffs, osc_iq, order=ORDER_AVX):
        super().__init__()
        c, o = _f32(coeffs), _f32(osc_iq).reshape(-1)
        if o.size % 2:
            raise SdrHipError("the oscillator table is interleaved (re, im) pairs")
        check(lib.sdrhip_tuner_create(C.byref(self.h), order, factor, _fp(c), c.size, _fp(o), o.size // 2), "sdrhip_tuner_create")
        self.factor = factor
        self.num_coeffs = lib.sdrhip_tuner_num_coeffs(self.h)
        self.period = lib.sdrhip_tuner_period(self.h)

    def set_route(self, route):
        check(lib.sdrhip_tuner_set_route(self.h, int(route)), "sdrhip_tuner_set_route")

    def run(self, d_in, in_base, d_out, k_begin, k_end, seam_block=0, stream=None):
        check(lib.sdrhip_tuner_run(self.h, stream, d_in, in_base, d_out, k_begin, k_end, seam_block), "sdrhip_tuner_run")

    def run_u8(self, d_in, in_base, d_out, k_begin, k_end, seam_block=0, stream=None):
        check(lib.sdrhip_tuner_run_u8(self.h, stream, d_in, in_base, d_out, k_begin, k_end, seam_block), "sdrhip_tuner_run_u8")

    def run_i16(self, d_in, in_base, d_out, k_begin, k_end, seam_block=0, stream=None):
        """interleaved int16 IQ input (4 bytes per sample), converted by s / 2048 in the kernels' loaders."""
        check(lib.sdrhip_tuner_run_i16(self.h, stream, d_in, in_base, d_out, k_begin, k_end, seam_block), "sdrhip_tuner_run_i16")


def tuner_i16_launches():
    """Launches of the int16 tile kernel so far, from a bank or a one-row tuner (sdrhip_debug_tuner_i16_launches)."""
    return int(lib.sdrhip_debug_tuner_i16_launches())


def tuner_bank_launches():
    """Banked launches of the tuner bank so far (sdrhip_debug_tuner_bank_launches)."""
    return int(lib.sdrhip_debug_tuner_bank_launches())


def tuner_bank_cross_launches():
    """Launches of the all-Cross kernel of the bank's Pipe so far (sdrhip_debug_tuner_bank_cross_launches)."""
    return int(lib.sdrhip_debug_tuner_bank_cross_launches())


class TunerBank(_Handle):
    """Every channel of one capture as complex baseband rows: K Tuners of the same decimator over ONE input, one launch per run where
    the banked route fits (sdr_hip.h, sdrhip_tuner_bank_*).  tables: one interleaved float32 (re, im) table per channel
    (tuner_shift_table builds the usual ones; a channel on the centre frequency takes [1, 0]).  Row j of a run is, bit for bit, what
    Tuner(factor, coeffs, tables[j], order) writes for the same launch."""
    _destroy = lib.sdrhip_tuner_bank_destroy
    ROUTE_AUTO, ROUTE_BANKED, ROUTE_CHANNELS = 0, 1, 2
    complex = True

    def __init__(self, factor, coeffs, tables, order=ORDER_AVX):
        super().__init__()
        c = _f32(coeffs)
        ts = [_f32(t).reshape(-1) for t in tables]
        if any(t.size % 2 for t in ts):
            raise SdrHipError("an oscillator table is interleaved (re, im) pairs")
        ptrs = (_f32p * max(len(ts), 1))(*[_fp(t) for t in ts])
        periods = (C.c_int * max(len(ts), 1))(*[t.size // 2 for t in ts])
        check(lib.sdrhip_tuner_bank_create(C.byref(self.h), order, factor, _fp(c), c.size, len(ts), ptrs, periods), "sdrhip_tuner_bank_create")
        self.factor = lib.sdrhip_tuner_bank_factor(self.h)
        self.num_coeffs = lib.sdrhip_tuner_bank_num_coeffs(self.h)

    @property
    def channels(self):
        return check(lib.sdrhip_tuner_bank_channels(self.h), "sdrhip_tuner_bank_channels")

    def period(self, channel):
        return check(lib.sdrhip_tuner_bank_period(self.h, int(channel)), "sdrhip_tuner_bank_period")

    def set_route(self, route):
        """0 = auto (the banked launch where it fits and was measured ahead of K tuner runs: sdr_hip.h), 1 = the banked launch (a
        launch it does not serve is an error), 2 = channel by channel."""
        check(lib.sdrhip_tuner_bank_set_route(self.h, int(route)), "sdrhip_tuner_bank_set_route")

    def run(self, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block=0, stream=None):
        """cfloat input; channel j's outputs [k_begin, k_end) -> d_out + 4 * j * out_stride bytes."""
        check(lib.sdrhip_tuner_bank_run(self.h, stream, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block), "sdrhip_tuner_bank_run")

    def run_u8(self, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block=0, stream=None):
        check(lib.sdrhip_tuner_bank_run_u8(self.h, stream, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block),
              "sdrhip_tuner_bank_run_u8")

    def run_i16(self, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block=0, stream=None):
        """interleaved int16 IQ input (4 bytes per sample); rows as run."""
        check(lib.sdrhip_tuner_bank_run_i16(self.h, stream, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block),
              "sdrhip_tuner_bank_run_i16")


def am_bank_launches():
    """Envelope tile launches of the AM bank's fused route so far (sdrhip_debug_am_bank_launches)."""
    return int(lib.sdrhip_debug_am_bank_launches())


def am_bank_fixup_launches():
    """Envelope fix-up launches of the AM bank's fused route so far (sdrhip_debug_am_bank_fixup_launches)."""
    return int(lib.sdrhip_debug_am_bank_fixup_launches())


def am_bank_cross_launches():
    """Launches of the all-Cross envelope kernel of the AM bank's Pipe so far (sdrhip_debug_am_bank_cross_launches)."""
    return int(lib.sdrhip_debug_am_bank_cross_launches())


class AmBank(_Handle):
    """The AM receiver for every channel of a TunerBank: row j of a run is the envelope (Data.Complex magnitude) of the bank's complex
    row j and, with dc_block, dcBlocker of that from the state in dc_state (2 K device floats, read and written; it belongs to output
    k_begin, so consecutive runs over consecutive ranges on one state array are one stream).  Bit for bit TunerBank.run ->
    am_demod_run_rows -> dc_blocker_run_rows on every route (sdr_hip.h, sdrhip_am_bank_*).  The tuner bank is borrowed: the object
    keeps a reference to it."""
    _destroy = lib.sdrhip_am_bank_destroy
    ROUTE_AUTO, ROUTE_FUSED, ROUTE_COMPOSED = 0, 1, 2

    def __init__(self, tuner_bank, dc_block=True):
        super().__init__()
        self.tuner_bank = tuner_bank
        self.dc_block = bool(dc_block)
        check(lib.sdrhip_am_bank_create(C.byref(self.h), tuner_bank.h, int(self.dc_block)), "sdrhip_am_bank_create")

    @property
    def channels(self):
        return check(lib.sdrhip_am_bank_channels(self.h), "sdrhip_am_bank_channels")

    def set_route(self, route):
        """0 = auto (sdr_hip.h), 1 = fused: the envelope form of the banked launch (a launch it does not serve is an error),
        2 = composed: the three calls of the definition."""
        check(lib.sdrhip_am_bank_set_route(self.h, int(route)), "sdrhip_am_bank_set_route")

    def workspace_bytes(self, count):
        return int(lib.sdrhip_am_bank_workspace_bytes(self.h, int(count)))

    def _run(self, fn, name, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block, dc_state, workspace, workspace_bytes, stream):
        check(fn(self.h, stream, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block, dc_state, workspace, workspace_bytes), name)

    def run(self, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block=0, dc_state=None, workspace=None, workspace_bytes=0,
            stream=None):
        """cfloat input; channel j's floats [k_begin, k_end) -> d_out + 4 * j * out_stride bytes.  Pointers are device addresses."""
        self._run(lib.sdrhip_am_bank_run, "sdrhip_am_bank_run", d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block, dc_state,
                  workspace, workspace_bytes, stream)

    def run_u8(self, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block=0, dc_state=None, workspace=None, workspace_bytes=0,
               stream=None):
        self._run(lib.sdrhip_am_bank_run_u8, "sdrhip_am_bank_run_u8", d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block,
                  dc_state, workspace, workspace_bytes, stream)

    def run_i16(self, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block=0, dc_state=None, workspace=None, workspace_bytes=0,
                stream=None):
        """interleaved int16 IQ input (4 bytes per sample); rows as run."""
        self._run(lib.sdrhip_am_bank_run_i16, "sdrhip_am_bank_run_i16", d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block,
                  dc_state, workspace, workspace_bytes, stream)


def nfm_bank_launches():
    """fmDemod-form tile launches of the narrow-band FM bank's fused route so far (sdrhip_debug_nfm_bank_launches)."""
    return int(lib.sdrhip_debug_nfm_bank_launches())


def nfm_bank_cross_launches():
    """Launches of the all-Cross fmDemod-form kernel of the narrow-band FM bank's Pipe so far (sdrhip_debug_nfm_bank_cross_launches)."""
    return int(lib.sdrhip_debug_nfm_bank_cross_launches())


class NfmBank(_Handle):
    """fmDemod for every channel of a TunerBank: row j of a run is phase(y[k] * conj y[k - 1]) over the bank's complex row j, the
    predecessor of output k_begin taken from `state` (K (re, im) pairs of device floats; None = zeros, the start of a stream) and
    output k_end - 1 left in `final` (None = not wanted; the two must not overlap).  Consecutive runs over consecutive ranges that
    swap the two arrays are one stream.  Bit for bit TunerBank.run -> fm_demod_run_rows on every route (sdr_hip.h,
    sdrhip_nfm_bank_*).  The tuner bank is borrowed: the object keeps a reference to it."""
    _destroy = lib.sdrhip_nfm_bank_destroy
    ROUTE_AUTO, ROUTE_FUSED, ROUTE_COMPOSED = 0, 1, 2

    def __init__(self, tuner_bank):
        super().__init__()
        self.tuner_bank = tuner_bank
        check(lib.sdrhip_nfm_bank_create(C.byref(self.h), tuner_bank.h), "sdrhip_nfm_bank_create")

    @property
    def channels(self):
        return check(lib.sdrhip_nfm_bank_channels(self.h), "sdrhip_nfm_bank_channels")

    def set_route(self, route):
        """0 = auto (sdr_hip.h), 1 = fused: ONE fmDemod-form launch of the banked tile kernel (a launch it does not serve is an
        error), 2 = composed: the two calls of the definition."""
        check(lib.sdrhip_nfm_bank_set_route(self.h, int(route)), "sdrhip_nfm_bank_set_route")

    def workspace_bytes(self, count):
        return int(lib.sdrhip_nfm_bank_workspace_bytes(self.h, int(count)))

    def _run(self, fn, name, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block, state, final, workspace, workspace_bytes, stream):
        check(fn(self.h, stream, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block, state, final, workspace, workspace_bytes), name)

    def run(self, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block=0, state=None, final=None, workspace=None,
            workspace_bytes=0, stream=None):
        """cfloat input; channel j's floats [k_begin, k_end) -> d_out + 4 * j * out_stride bytes.  Pointers are device addresses."""
        self._run(lib.sdrhip_nfm_bank_run, "sdrhip_nfm_bank_run", d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block, state,
                  final, workspace, workspace_bytes, stream)

    def run_u8(self, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block=0, state=None, final=None, workspace=None,
               workspace_bytes=0, stream=None):
        self._run(lib.sdrhip_nfm_bank_run_u8, "sdrhip_nfm_bank_run_u8", d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block,
                  state, final, workspace, workspace_bytes, stream)

    def run_i16(self, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block=0, state=None, final=None, workspace=None,
                workspace_bytes=0, stream=None):
        """interleaved int16 IQ input (4 bytes per sample); rows as run."""
        self._run(lib.sdrhip_nfm_bank_run_i16, "sdrhip_nfm_bank_run_i16", d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block,
                  state, final, workspace, workspace_bytes, stream)


NARROW_ENV, NARROW_FM = 0, 1


def narrow_bank_launches():
    """Launches of the narrow-channel bank's kernel so far: one per run on its fused route (sdrhip_debug_narrow_bank_launches)."""
    return int(lib.sdrhip_debug_narrow_bank_launches())


def narrow_bank_tile(form):
    """Outputs a tile of the narrow-channel bank's kernel advances by: 256 for NARROW_ENV, 255 for NARROW_FM."""
    return int(lib.sdrhip_debug_narrow_bank_tile(int(form)))


class NarrowBank(_Handle):
    """A second complex decimator and the demodulator behind every channel of a TunerBank: row j of a run holds the stage-2 outputs
    [k_begin, k_end) of  TunerBank.run -> Decimator.run_rows -> am_demod_rows | fm_demod_rows [-> dc_blocker_rows], bit for bit on
    every route (sdr_hip.h, sdrhip_narrow_bank_*).  form: NARROW_ENV (magnitude; dc_block adds dcBlocker from `dc_state`, 2 K device
    floats that belong to output k_begin) or NARROW_FM (fmDemod; `state` / `final` as NfmBank's, of STAGE-2 outputs).  seam_block is
    the first decimator Pipe's block in input samples, seam_block2 the second one's in stage-1 outputs.  Tuner bank and decimator
    are borrowed: the object keeps references to them."""
    _destroy = lib.sdrhip_narrow_bank_destroy
    ROUTE_AUTO, ROUTE_FUSED, ROUTE_COMPOSED = 0, 1, 2

    def __init__(self, tuner_bank, decimator, form, dc_block=False):
        super().__init__()
        self.tuner_bank = tuner_bank
        self.decimator = decimator
        self.form = int(form)
        self.dc_block = bool(dc_block)
        check(lib.sdrhip_narrow_bank_create(C.byref(self.h), tuner_bank.h, decimator.h, self.form, int(self.dc_block)),
              "sdrhip_narrow_bank_create")

    @property
    def channels(self):
        return check(lib.sdrhip_narrow_bank_channels(self.h), "sdrhip_narrow_bank_channels")

    def set_route(self, route):
        """0 = auto (sdr_hip.h), 1 = fused: the tuner bank, then ONE launch of the narrow kernel (a run it does not serve is an
        error), 2 = composed: the calls of the definition."""
        check(lib.sdrhip_narrow_bank_set_route(self.h, int(route)), "sdrhip_narrow_bank_set_route")

    def workspace_bytes(self, count):
        """For the current route setting; route 2's figure serves every route."""
        return int(lib.sdrhip_narrow_bank_workspace_bytes(self.h, int(count)))

    def stage1_range(self, k_begin, k_end):
        """(j_begin, j_end): the stage-1 outputs that stage-2 outputs [k_begin, k_end) read."""
        j0, j1 = _i64(0), _i64(0)
        check(lib.sdrhip_narrow_bank_stage1_range(self.h, int(k_begin), int(k_end), C.byref(j0), C.byref(j1)),
              "sdrhip_narrow_bank_stage1_range")
        return int(j0.value), int(j1.value)

    def _run(self, fn, name, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block, seam_block2, state, final, dc_state, workspace,
             workspace_bytes, stream):
        check(fn(self.h, stream, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block, seam_block2, state, final, dc_state, workspace,
                 workspace_bytes), name)

    def run(self, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block=0, seam_block2=0, state=None, final=None, dc_state=None,
            workspace=None, workspace_bytes=0, stream=None):
        """cfloat input; channel j's floats [k_begin, k_end) -> d_out + 4 * j * out_stride bytes.  Pointers are device addresses."""
        self._run(lib.sdrhip_narrow_bank_run, "sdrhip_narrow_bank_run", d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block,
                  seam_block2, state, final, dc_state, workspace, workspace_bytes, stream)

    def run_u8(self, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block=0, seam_block2=0, state=None, final=None, dc_state=None,
               workspace=None, workspace_bytes=0, stream=None):
        self._run(lib.sdrhip_narrow_bank_run_u8, "sdrhip_narrow_bank_run_u8", d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block,
                  seam_block2, state, final, dc_state, workspace, workspace_bytes, stream)

    def run_i16(self, d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block=0, seam_block2=0, state=None, final=None, dc_state=None,
                workspace=None, workspace_bytes=0, stream=None):
        """interleaved int16 IQ input (4 bytes per sample); rows as run."""
        self._run(lib.sdrhip_narrow_bank_run_i16, "sdrhip_narrow_bank_run_i16", d_in, in_base, d_out, out_stride, k_begin, k_end, seam_block,
                  seam_block2, state, final, dc_state, workspace, workspace_bytes, stream)


class FmChain(_Handle):
    """The FM receiver of examples/fm/fm.hs:34-41 as one device-resident object."""
    _destroy = lib.sdrhip_fm_chain_destroy

    def __init__(self, decim_factor, decim_taps, interpolation, decimation, resamp_taps, audio_half_taps,
                 gain=1.0, block=8192, order=ORDER_AVX):
        super().__init__()
        a, b, c = _f32(decim_taps), _f32(resamp_taps), _f32(audio_half_taps)
        check(lib.sdrhip_fm_chain_create(C.byref(self.h), order, decim_factor, _fp(a), a.size, interpolation,
                                         decimation, _fp(b), b.size, _fp(c), c.size, C.c_float(gain), block),
              "sdrhip_fm_chain_create")

    def plan(self, s0, s1, total_in=-1):
        q0, q1, halo = _i64(), _i64(), _i64()
        check(lib.sdrhip_fm_chain_plan(self.h, s0, s1, total_in, C.byref(q0), C.byref(q1), C.byref(halo)), "sdrhip_fm_chain_plan")
        return q0.value, q1.value, halo.value

    def ready(self, n_samples):
        """Audio outputs computable from the first n_samples samples of the stream."""
        return int(lib.sdrhip_fm_chain_ready(self.h, n_samples))

    def max_halo(self):
        return lib.sdrhip_fm_chain_max_halo(self.h)

    def halo_staging_bytes(self, count):
        return int(lib.sdrhip_fm_chain_halo_staging_bytes(self.h, count))

    def halo_samples(self):
        """max_halo rounded up to whole 16-byte vectors: the size of the halo message, the same on every rank."""
        return int(lib.sdrhip_fm_chain_halo_samples(self.h))

    def workspace_bytes(self, n_in):
        return lib.sdrhip_fm_chain_workspace_bytes(self.h, n_in)

    STAGES = ("decimate", "fm_demod", "resample", "filter", "fused_tail", "fused_chain")

    def set_overlap(self, on):
        """Two runs in flight: consecutive runs alternate between two internal streams and workspace halves (sdr_hip.h)."""
        check(lib.sdrhip_fm_chain_set_overlap(self.h, 1 if on else 0), "sdrhip_fm_chain_set_overlap")

    def join(self, stream=0):
        check(lib.sdrhip_fm_chain_join(self.h, stream), "sdrhip_fm_chain_join")

    def set_fused_tail(self, mode=2):
        """0 = stage kernels, 1 = the fused tail kernel wherever the chain's shape allows, 2 = auto (short runs only)."""
        check(lib.sdrhip_fm_chain_set_fused_tail(self.h, int(mode)), "sdrhip_fm_chain_set_fused_tail")

    def set_small_chain(self, mode=2, max_outputs=0, tile_outputs=0):
        """0 = never, 1 = always, 2 = auto: the whole chain as one kernel for launch-bound runs (kernels_small.hip)."""
        check(lib.sdrhip_fm_chain_set_small_chain(self.h, int(mode), int(max_outputs), int(tile_outputs)), "sdrhip_fm_chain_set_small_chain")

    def set_tuner(self, osc_iq=None):
        """`P.map (VG.zipWith (*) osc)` in front of the chain's decimator (sdrhip_fm_chain_set_tuner): osc_iq = interleaved float32
        (re, im) pairs, indexed by the absolute stream position mod their count (tuner_shift_table builds the usual tables);
        None removes the tuner.  No run of the chain may be in flight; graphs and workspaces made before are made again."""
        if osc_iq is None:
            check(lib.sdrhip_fm_chain_set_tuner(self.h, None, 0), "sdrhip_fm_chain_set_tuner")
            return
        o = _f32(osc_iq).reshape(-1)
        if o.size % 2:
            raise SdrHipError("the oscillator table is interleaved (re, im) pairs")
        check(lib.sdrhip_fm_chain_set_tuner(self.h, _fp(o), o.size // 2), "sdrhip_fm_chain_set_tuner")

    def tuner_period(self):
        """Entries of the tuner's table, 0 = no tuner."""
        return check(lib.sdrhip_fm_chain_tuner_period(self.h), "sdrhip_fm_chain_tuner_period")

    def set_demod_fusion(self, on=True):
        """fmDemod inside the resampler's tile loader on large batches (sdrhip_fm_chain_set_demod_fusion)."""
        check(lib.sdrhip_fm_chain_set_demod_fusion(self.h, int(on)), "sdrhip_fm_chain_set_demod_fusion")

    def enable_timing(self, on=True):
        check(lib.sdrhip_fm_chain_enable_timing(self.h, int(on)), "sdrhip_fm_chain_enable_timing")

    def read_timing(self):
        """-> (dict stage -> mean ms per run, runs)"""
        ms = (C.c_double * 6)()
        runs = C.c_int()
        check(lib.sdrhip_fm_chain_read_timing(self.h, ms, C.byref(runs)), "sdrhip_fm_chain_read_timing")
        n = max(runs.value, 1)
        return {k: ms[i] / n for i, k in enumerate(self.STAGES)}, runs.value

    def run(self, d_in_u8, s0, n_in, d_audio, q0, q1, d_ws, ws_bytes, stream=None):
        check(lib.sdrhip_fm_chain_run(self.h, stream, d_in_u8, s0, n_in, d_audio, q0, q1, d_ws, ws_bytes), "sdrhip_fm_chain_run")


def fm_bank_launches():
    """Banked launches so far (sdrhip_debug_fm_bank_launches)."""
    return int(lib.sdrhip_debug_fm_bank_launches())


def fm_bank_i16_launches():
    """Banked launches on int16 input so far (sdrhip_debug_fm_bank_i16_launches); each counts in fm_bank_launches() too."""
    return int(lib.sdrhip_debug_fm_bank_i16_launches())


class FmBank(_Handle):
    """Every station of one capture: K tuned FmChains of the same arguments over ONE input, one launch per run where the banked route
    fits (sdr_hip.h, sdrhip_fm_bank_*).  tables: one interleaved float32 (re, im) table per station (tuner_shift_table builds the
    usual ones; a station on the centre frequency takes [1, 0]).  Row j of a run is, bit for bit, what
    FmChain(...).set_tuner(tables[j]) writes."""
    _destroy = lib.sdrhip_fm_bank_destroy
    ROUTE_AUTO, ROUTE_BANKED, ROUTE_STATIONS = 0, 1, 2

    def __init__(self, decim_factor, decim_taps, interpolation, decimation, resamp_taps, audio_half_taps, tables,
                 gain=1.0, block=8192, order=ORDER_AVX):
        super().__init__()
        a, b, c = _f32(decim_taps), _f32(resamp_taps), _f32(audio_half_taps)
        ts = [_f32(t).reshape(-1) for t in tables]
        if any(t.size % 2 for t in ts):
            raise SdrHipError("an oscillator table is interleaved (re, im) pairs")
        ptrs = (_f32p * max(len(ts), 1))(*[_fp(t) for t in ts])
        periods = (C.c_int * max(len(ts), 1))(*[t.size // 2 for t in ts])
        check(lib.sdrhip_fm_bank_create(C.byref(self.h), order, decim_factor, _fp(a), a.size, interpolation, decimation, _fp(b), b.size,
                                        _fp(c), c.size, C.c_float(gain), block, len(ts), ptrs, periods), "sdrhip_fm_bank_create")

    def stations(self):
        return check(lib.sdrhip_fm_bank_stations(self.h), "sdrhip_fm_bank_stations")

    def period(self, station):
        return check(lib.sdrhip_fm_bank_period(self.h, int(station)), "sdrhip_fm_bank_period")

    def plan(self, s0, s1, total_in=-1):
        q0, q1, halo = _i64(), _i64(), _i64()
        check(lib.sdrhip_fm_bank_plan(self.h, s0, s1, total_in, C.byref(q0), C.byref(q1), C.byref(halo)), "sdrhip_fm_bank_plan")
        return q0.value, q1.value, halo.value

    def ready(self, n_samples):
        return int(lib.sdrhip_fm_bank_ready(self.h, n_samples))

    def max_halo(self):
        return int(lib.sdrhip_fm_bank_max_halo(self.h))

    def workspace_bytes(self, n_in):
        return int(lib.sdrhip_fm_bank_workspace_bytes(self.h, n_in))

    def set_route(self, route=0, max_outputs=0, tile_outputs=0):
        """0 = auto, 1 = the banked one-kernel launch (a run it does not fit is an error), 2 = station by station.  Auto is a rule
        in two dimensions: the banked launch while a station's run is at most 39322 outputs (2^20 samples; fixed) AND stations * outputs
        <= max_outputs (0 = built-in, 32 * 39322); longer runs go station by station whatever the number of stations.  tile_outputs
        as FmChain.set_small_chain."""
        check(lib.sdrhip_fm_bank_set_route(self.h, int(route), int(max_outputs), int(tile_outputs)), "sdrhip_fm_bank_set_route")

    def run(self, d_in_u8, s0, n_in, d_audio, audio_stride, q0, q1, d_ws=None, ws_bytes=0, stream=None):
        """Station j's outputs [q0, q1) -> d_audio + 4 * j * audio_stride bytes."""
        check(lib.sdrhip_fm_bank_run(self.h, stream, d_in_u8, s0, n_in, d_audio, audio_stride, q0, q1, d_ws, ws_bytes), "sdrhip_fm_bank_run")

    def run_i16(self, d_in_i16, s0, n_in, d_audio, audio_stride, q0, q1, d_ws=None, ws_bytes=0, stream=None):
        """run on 16-bit signed IQ (interleaved int16, 4 bytes per sample; sdrhip_fm_bank_run_i16): row j is, bit for bit,
        Tuner.run_i16 -> fm_demod -> Resampler.run -> Filter.run -> scale driven by hand with table j."""
        check(lib.sdrhip_fm_bank_run_i16(self.h, stream, d_in_i16, s0, n_in, d_audio, audio_stride, q0, q1, d_ws, ws_bytes), "sdrhip_fm_bank_run_i16")


class Fft(_Handle):
    """fftw' / fftwReal' of SDR.FFT (FFT.hs:44-108) on hipFFT: Complex Double in FFTW's order, `batch` transforms per call."""
    _destroy = lib.sdrhip_fft_destroy

    def __init__(self, n, real_input=False, batch=1):
        super().__init__()
        check(lib.sdrhip_fft_create(C.byref(self.h), n, int(real_input), batch), "sdrhip_fft_create")
        self.n, self.real_input, self.batch = n, bool(real_input), batch
        self.bins = lib.sdrhip_fft_bins(self.h)

    def run(self, x):
        import numpy as np
        if self.real_input:
            a = np.ascontiguousarray(x, dtype=np.float64).reshape(self.batch, self.n)
        else:
            a = np.ascontiguousarray(x, dtype=np.complex128).reshape(self.batch, self.n)
        out = np.empty((self.batch, self.bins), np.complex128)
        check(lib.sdrhip_fft_run(self.h, a.ctypes.data_as(_f64p), out.ctypes.data_as(_f64p)), "sdrhip_fft_run")
        return out if self.batch > 1 else out[0]


IQ_U8, IQ_CF32, IQ_I16 = 0, 1, 2
WINDOW_NONE, WINDOW_HANNING, WINDOW_HAMMING, WINDOW_BLACKMAN, WINDOW_CUSTOM = 0, 1, 2, 3, 4
SPECTRUM_ROUTE_AUTO, SPECTRUM_ROUTE_FUSED, SPECTRUM_ROUTE_HIPFFT = 0, 1, 2
REDUCE_MEAN_POWER, REDUCE_MEAN_MAGNITUDE, REDUCE_MAX_MAGNITUDE = 0, 1, 2
UNIT_LINEAR, UNIT_DB = 0, 1
REDUCE_SPLIT_AUTO, REDUCE_SPLIT_NEVER, REDUCE_SPLIT_ALWAYS = 0, 1, 2


class Spectrum(_Handle):
    """The reference's waterfall pipe as one operator: raw IQ (u8, interleaved float32 or interleaved int16) x halfBandUp x window -> DFT ->
    scale * |X| as float32 rows (sdr_hip.h, sdrhip_spectrum_*).  Row r covers samples [r*hop, r*hop + n)."""
    _destroy = lib.sdrhip_spectrum_destroy

    def __init__(self, n, input_format=IQ_U8, window=WINDOW_NONE, half_band_shift=False, scale=1.0, custom_window=None):
        super().__init__()
        import numpy as np
        cw = None
        if custom_window is not None:
            cw = np.ascontiguousarray(custom_window, dtype=np.float64)
            if cw.size != n:
                raise SdrHipError(f"a custom window of {cw.size} values for n = {n}")
        check(lib.sdrhip_spectrum_create(C.byref(self.h), n, input_format, window, cw.ctypes.data_as(_f64p) if cw is not None else None,
                                         int(bool(half_band_shift)), float(scale)), "sdrhip_spectrum_create")
        self.n, self.input_format = n, input_format

    def _host_dtype(self):
        import numpy as np
        return {IQ_U8: np.uint8, IQ_I16: np.int16}.get(self.input_format, np.float32)

    def window(self):
        import numpy as np
        w = np.empty(self.n, np.float64)
        check(lib.sdrhip_spectrum_window(self.h, w.ctypes.data_as(_f64p)), "sdrhip_spectrum_window")
        return w

    def set_route(self, route):
        check(lib.sdrhip_spectrum_set_route(self.h, int(route)), "sdrhip_spectrum_set_route")

    def rows_of(self, n_samples, hop):
        """Whole rows a buffer of n_samples holds at this hop."""
        return 0 if n_samples < self.n else (n_samples - self.n) // hop + 1

    def run_device(self, d_in, n_samples, d_out, hop=None, rows=None, stream=None):
        """d_in, d_out: device addresses; d_out takes rows x n float32."""
        hop = self.n if hop is None else int(hop)
        rows = self.rows_of(n_samples, hop) if rows is None else int(rows)
        check(lib.sdrhip_spectrum_run_device(self.h, stream, d_in, n_samples, hop, rows, d_out), "sdrhip_spectrum_run_device")
        return rows

    def run(self, iq, hop=None, rows=None):
        """iq: a host array of interleaved samples (uint8, float32 or int16, by input_format) -> rows x n float32."""
        import numpy as np
        a = np.ascontiguousarray(iq, dtype=self._host_dtype()).reshape(-1)
        n_samples = a.size // 2
        hop = self.n if hop is None else int(hop)
        rows = self.rows_of(n_samples, hop) if rows is None else int(rows)
        out = np.empty((max(rows, 0), self.n), np.float32)
        check(lib.sdrhip_spectrum_run(self.h, a.ctypes.data, n_samples, hop, rows, out.ctypes.data), "sdrhip_spectrum_run")
        return out

    def set_reduce_split(self, mode):
        check(lib.sdrhip_spectrum_set_reduce_split(self.h, int(mode)), "sdrhip_spectrum_set_reduce_split")

    def reduce_device(self, d_in, n_samples, d_out, group, reduce=REDUCE_MEAN_POWER, unit=UNIT_LINEAR, floor_db=-200.0, hop=None, rows_out=None,
                      stream=None):
        """d_in, d_out: device addresses; d_out takes rows_out x n float32, output row R reducing input rows R*group .. R*group+group-1
        (mean power, mean magnitude or max; linear or dB, never below floor_db).  -> rows_out."""
        hop = self.n if hop is None else int(hop)
        rows_out = self.rows_of(n_samples, hop) // int(group) if rows_out is None else int(rows_out)
        check(lib.sdrhip_spectrum_reduce_run_device(self.h, stream, d_in, n_samples, hop, rows_out, int(group), int(reduce), int(unit),
                                                    float(floor_db), d_out), "sdrhip_spectrum_reduce_run_device")
        return rows_out

    def reduce(self, iq, group, reduce=REDUCE_MEAN_POWER, unit=UNIT_LINEAR, floor_db=-200.0, hop=None, rows_out=None):
        """iq: a host array of interleaved samples -> rows_out x n float32 (see reduce_device)."""
        import numpy as np
        a = np.ascontiguousarray(iq, dtype=self._host_dtype()).reshape(-1)
        n_samples = a.size // 2
        hop = self.n if hop is None else int(hop)
        rows_out = self.rows_of(n_samples, hop) // int(group) if rows_out is None else int(rows_out)
        out = np.empty((max(rows_out, 0), self.n), np.float32)
        check(lib.sdrhip_spectrum_reduce_run(self.h, a.ctypes.data, n_samples, hop, rows_out, int(group), int(reduce), int(unit), float(floor_db),
                                             out.ctypes.data), "sdrhip_spectrum_reduce_run")
        return out


def spectrum_fused_launches():
    return int(lib.sdrhip_debug_spectrum_fused_launches())


def spectrum_reduce_split_launches():
    return int(lib.sdrhip_debug_spectrum_reduce_split_launches())


def spectrum_hipfft_batches():
    return int(lib.sdrhip_debug_spectrum_hipfft_batches())


def spectrum_reduce_layer_launches():
    return int(lib.sdrhip_debug_spectrum_reduce_layer_launches())


TRANSPORT_RCCL, TRANSPORT_PEER_COPY = 1, 2
COMM_ID_BYTES = 128


def comm_unique_id():
    """The 128-byte rendezvous id rank 0 creates (ncclGetUniqueId) and hands to the other ranks out of band."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    check(lib.sdrhip_comm_get_unique_id(buf), "sdrhip_comm_get_unique_id")
    return buf.raw


class Comm(_Handle):
    """One rank's communicator for the halo exchange (RCCL point-to-point inside libsdr_hip.so)."""
    _destroy = lib.sdrhip_comm_destroy

    def __init__(self, nranks=None, rank=None, uid=None, _adopt=None):
        super().__init__()
        if _adopt is not None:
            self.h = _adopt
            return
        check(lib.sdrhip_comm_init_rank(C.byref(self.h), nranks, rank, uid), "sdrhip_comm_init_rank")

    @staticmethod
    def local(devices, transport=TRANSPORT_RCCL):
        """All `devices` from this process: one Comm per device, rank i on devices[i]."""
        n = len(devices)
        hs = (_vp * n)()
        devs = (C.c_int * n)(*devices)
        check(lib.sdrhip_comm_init_local(hs, n, devs, transport), "sdrhip_comm_init_local")
        return [Comm(_adopt=_vp(hs[i])) for i in range(n)]

    @property
    def rank(self):
        return lib.sdrhip_comm_rank(self.h)

    @property
    def size(self):
        return lib.sdrhip_comm_size(self.h)

    @property
    def transport(self):
        return lib.sdrhip_comm_transport(self.h).decode()

    def halo_exchange(self, d_send, d_recv, nbytes, stream=None):
        check(lib.sdrhip_halo_exchange(self.h, stream, d_send, d_recv, nbytes), "sdrhip_halo_exchange")

    def chain_halo_exchange(self, chain, d_buf, shard_samples, stream=None):
        check(lib.sdrhip_fm_chain_halo_exchange(chain.h, self.h, stream, d_buf, shard_samples), "sdrhip_fm_chain_halo_exchange")

    def chain_halo_exchange_batch(self, chain, d_buf, shard_samples, row_bytes, count, d_staging, stream=None):
        """The halos of `count` consecutive super-blocks (rows of row_bytes at d_buf) in one message pair."""
        check(lib.sdrhip_fm_chain_halo_exchange_batch(chain.h, self.h, stream, d_buf, shard_samples, row_bytes, count, d_staging),
              "sdrhip_fm_chain_halo_exchange_batch")


def halo_exchange_all(comms, streams, d_send, d_recv, nbytes):
    n = len(comms)
    hs = (_vp * n)(*[c.h for c in comms])
    ss = (_vp * n)(*[_vp(s) for s in streams])
    sd = (_vp * n)(*[_vp(p) for p in d_send])
    rv = (_vp * n)(*[_vp(p) for p in d_recv])
    check(lib.sdrhip_halo_exchange_all(hs, n, ss, sd, rv, nbytes), "sdrhip_halo_exchange_all")


class FmGraph(_Handle):
    """One FmChain.run with fixed arguments as a hipGraph (sdrhip_fm_chain_graph_*): one launch per pass."""
    _destroy = lib.sdrhip_fm_chain_graph_destroy

    def __init__(self, chain, d_in_u8, s0, n_in, d_audio, q0, q1, d_ws, ws_bytes):
        super().__init__()
        self.chain = chain
        check(lib.sdrhip_fm_chain_graph_create(C.byref(self.h), chain.h, d_in_u8, s0, n_in, d_audio, q0, q1, d_ws, ws_bytes),
              "sdrhip_fm_chain_graph_create")

    def launch(self, stream=None):
        check(lib.sdrhip_fm_chain_graph_launch(self.h, stream), "sdrhip_fm_chain_graph_launch")


class FmStream(_Handle):
    """u8 IQ host blocks in, audio host blocks out: the FM receiver of fm.hs:34-41 as one operator.  Over an FmBank
    (sdrhip_fm_stream_create_bank) every station's audio comes out in lockstep: push, flush, poll and restore then return a list of
    arrays of shape [stations, block_size_out] -- row j is, bit for bit, the block an FmStream over FmChain(...).set_tuner(tables[j])
    yields -- where a chain's stream returns a list of [block_size_out] arrays.  input_i16=True (a bank only,
    sdrhip_fm_stream_create_bank_i16): the stream takes interleaved int16 IQ through push_i16 / input_buffer_i16."""
    _destroy = lib.sdrhip_fm_stream_destroy

    def __init__(self, chain, max_block_samples, block_size_out=8192, input_i16=False):
        super().__init__()
        self.chain = chain  # the chain or the bank: keep alive
        self.block_size_out = block_size_out
        self.is_bank = isinstance(chain, FmBank)
        self.input_i16 = bool(input_i16)
        if self.input_i16:
            if not self.is_bank:
                raise SdrHipError("FmStream(input_i16=True): int16 IQ reaches the FM side through an FmBank")
            check(lib.sdrhip_fm_stream_create_bank_i16(C.byref(self.h), chain.h, max_block_samples, block_size_out),
                  "sdrhip_fm_stream_create_bank_i16")
        elif self.is_bank:
            check(lib.sdrhip_fm_stream_create_bank(C.byref(self.h), chain.h, max_block_samples, block_size_out), "sdrhip_fm_stream_create_bank")
        else:
            check(lib.sdrhip_fm_stream_create(C.byref(self.h), chain.h, max_block_samples, block_size_out), "sdrhip_fm_stream_create")

    def rows(self):
        """1 for a chain's stream, the number of stations for a bank's."""
        return check(lib.sdrhip_fm_stream_rows(self.h), "sdrhip_fm_stream_rows")

    def pop_rows(self, max_blocks):
        """Up to max_blocks blocks of every station at once: an array [rows, nb, block_size_out] (sdrhip_fm_stream_pop_rows)."""
        rows, n = self.rows(), self.block_size_out
        o = np.empty((rows, max(max_blocks, 0) * n), np.float32)
        nb = check(lib.sdrhip_fm_stream_pop_rows(self.h, _fp(o), o.shape[1], max_blocks), "sdrhip_fm_stream_pop_rows")
        return o[:, : nb * n].reshape(rows, nb, n)

    def set_coalesce(self, samples):
        check(lib.sdrhip_fm_stream_set_coalesce(self.h, samples), "sdrhip_fm_stream_set_coalesce")

    def set_adaptive(self, max_samples):
        check(lib.sdrhip_fm_stream_set_adaptive(self.h, max_samples), "sdrhip_fm_stream_set_adaptive")

    def _pop(self, ready):
        if self.is_bank:
            if ready <= 0:
                return []
            got = self.pop_rows(ready)
            return [np.ascontiguousarray(got[:, k]) for k in range(got.shape[1])]
        outs = []
        for _ in range(ready):
            o = np.empty(self.block_size_out, np.float32)
            check(lib.sdrhip_fm_stream_pop(self.h, _fp(o), self.block_size_out), "sdrhip_fm_stream_pop")
            outs.append(o)
        return outs

    def push(self, u8_iq):
        b = np.ascontiguousarray(u8_iq, dtype=np.uint8)
        return self._pop(check(lib.sdrhip_fm_stream_push(self.h, b.ctypes.data_as(_u8p), b.size // 2), "sdrhip_fm_stream_push"))

    def input_buffer(self, n_samples):
        """numpy view of the pinned staging buffer of the next push (fill it, then push_inplace)."""
        p = lib.sdrhip_fm_stream_input_buffer(self.h)
        if not p:
            raise SdrHipError(lib.sdrhip_last_error().decode())
        return np.ctypeslib.as_array(C.cast(p, _u8p), shape=(2 * n_samples,))

    def push_inplace(self, view):
        return self._pop(check(lib.sdrhip_fm_stream_push(self.h, view.ctypes.data_as(_u8p), view.size // 2), "sdrhip_fm_stream_push"))

    def push_i16(self, i16_iq):
        """interleaved int16 IQ (a view input_buffer_i16 gave is pushed in place)"""
        b = np.ascontiguousarray(i16_iq, dtype=np.int16)
        return self._pop(check(lib.sdrhip_fm_stream_push_i16(self.h, b.ctypes.data_as(_vp), b.size // 2), "sdrhip_fm_stream_push_i16"))

    def input_buffer_i16(self, n_samples):
        """numpy int16 view of the pinned staging buffer of the next push (fill it, then push_i16 the view)."""
        p = lib.sdrhip_fm_stream_input_buffer_i16(self.h)
        if not p:
            raise SdrHipError(lib.sdrhip_last_error().decode())
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int16)), shape=(2 * n_samples,))

    def flush(self):
        return self._pop(check(lib.sdrhip_fm_stream_flush(self.h), "sdrhip_fm_stream_flush"))

    def poll(self):
        """blocks the GPU has finished meanwhile (never waits)"""
        return self._pop(check(lib.sdrhip_fm_stream_poll(self.h), "sdrhip_fm_stream_poll"))

    def save(self):
        """sdrhip_fm_stream_save: drains the operator and returns its state as bytes (audio blocks that became ready stay
        inside the state / the stream: pop them from either)."""
        lib.sdrhip_fm_stream_state_bytes.restype = C.c_size_t
        lib.sdrhip_fm_stream_state_bytes.argtypes = [C.c_void_p]
        cap = lib.sdrhip_fm_stream_state_bytes(self.h)                   # includes room for the audio the drain adds
        buf = (C.c_ubyte * cap)()
        used = C.c_size_t()
        lib.sdrhip_fm_stream_save.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        check(lib.sdrhip_fm_stream_save(self.h, buf, cap, C.byref(used)), "sdrhip_fm_stream_save")
        return bytes(buf[: used.value])

    def restore(self, state):
        lib.sdrhip_fm_stream_restore.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        return self._pop(check(lib.sdrhip_fm_stream_restore(self.h, state, len(state)), "sdrhip_fm_stream_restore"))


class Pipe(_Handle):
    """firFilter / firDecimator / firResampler / fmDemod / amDemod / dcBlockingFilter / agcPipe on host blocks (Filter.hs:532-739,
    Demod.hs:40-46, Util.hs:344-348).  Pipe.tuner_bank: every channel of a TunerBank in lockstep -- push, flush, poll and restore
    then return a list of arrays of shape [channels, 2 * block_size_out], row j being the block Pipe.tuner over
    Tuner(factor, coeffs, tables[j], order) yields."""
    _destroy = lib.sdrhip_pipe_destroy

    def __init__(self, kind, desc=None, block_size_out=8192, mu=None, reference=None, input_u8=False, input_i16=False, spectrum_args=None):
        super().__init__()
        self.desc = desc  # keep the descriptor alive
        self.block_size_out = block_size_out
        self.input_u8 = False
        self.input_i16 = False
        self.complex_in = bool(getattr(desc, "complex", False)) or kind in ("fm_demod", "am_demod", "agc")
        self.complex_out = bool(getattr(desc, "complex", False)) or kind == "agc"
        if kind == "filter":
            check(lib.sdrhip_pipe_fir_filter(C.byref(self.h), desc.h, block_size_out), "sdrhip_pipe_fir_filter")
        elif kind == "decimator":
            check(lib.sdrhip_pipe_fir_decimator(C.byref(self.h), desc.h, block_size_out), "sdrhip_pipe_fir_decimator")
        elif kind == "resampler":
            check(lib.sdrhip_pipe_fir_resampler(C.byref(self.h), desc.h, block_size_out), "sdrhip_pipe_fir_resampler")
        elif kind == "tuner":
            check(lib.sdrhip_pipe_tuner(C.byref(self.h), desc.h, block_size_out), "sdrhip_pipe_tuner")
        elif kind == "tuner_bank" and input_i16:
            if input_u8:
                raise ValueError("Pipe.tuner_bank: input_u8 and input_i16 exclude each other")
            check(lib.sdrhip_pipe_tuner_bank_i16(C.byref(self.h), desc.h, block_size_out), "sdrhip_pipe_tuner_bank_i16")
            self.input_i16 = True
        elif kind == "tuner_bank":
            check(lib.sdrhip_pipe_tuner_bank(C.byref(self.h), desc.h, block_size_out, int(input_u8)), "sdrhip_pipe_tuner_bank")
            self.input_u8 = bool(input_u8)
        elif kind == "am_bank":
            if input_u8 and input_i16:
                raise ValueError("Pipe.am_bank: input_u8 and input_i16 exclude each other")
            check(lib.sdrhip_pipe_am_bank(C.byref(self.h), desc.h, block_size_out, 2 if input_i16 else int(bool(input_u8))), "sdrhip_pipe_am_bank")
            self.input_u8, self.input_i16 = bool(input_u8), bool(input_i16)
            self.complex_in = True
        elif kind == "nfm_bank":
            if input_u8 and input_i16:
                raise ValueError("Pipe.nfm_bank: input_u8 and input_i16 exclude each other")
            check(lib.sdrhip_pipe_nfm_bank(C.byref(self.h), desc.h, block_size_out, 2 if input_i16 else int(bool(input_u8))), "sdrhip_pipe_nfm_bank")
            self.input_u8, self.input_i16 = bool(input_u8), bool(input_i16)
            self.complex_in = True
        elif kind in ("am_bank_audio", "nfm_bank_audio"):
            if input_u8 and input_i16:
                raise ValueError(f"Pipe.{kind}: input_u8 and input_i16 exclude each other")
            bank, tail = desc
            fn = lib.sdrhip_pipe_am_bank_audio if kind == "am_bank_audio" else lib.sdrhip_pipe_nfm_bank_audio
            check(fn(C.byref(self.h), bank.h, tail.h, 2 if input_i16 else int(bool(input_u8))), "sdrhip_pipe_" + kind)
            self.input_u8, self.input_i16 = bool(input_u8), bool(input_i16)
            self.complex_in = True
        elif kind == "narrow_bank":
            if input_u8 and input_i16:
                raise ValueError("Pipe.narrow_bank: input_u8 and input_i16 exclude each other")
            bank, block_mid = desc
            check(lib.sdrhip_pipe_narrow_bank(C.byref(self.h), bank.h, int(block_mid), block_size_out, 2 if input_i16 else int(bool(input_u8))),
                  "sdrhip_pipe_narrow_bank")
            self.input_u8, self.input_i16 = bool(input_u8), bool(input_i16)
            self.complex_in = True
        elif kind == "narrow_bank_audio":
            if input_u8 and input_i16:
                raise ValueError("Pipe.narrow_bank_audio: input_u8 and input_i16 exclude each other")
            bank, tail, block_mid = desc
            check(lib.sdrhip_pipe_narrow_bank_audio(C.byref(self.h), bank.h, tail.h, int(block_mid), 2 if input_i16 else int(bool(input_u8))),
                  "sdrhip_pipe_narrow_bank_audio")
            self.input_u8, self.input_i16 = bool(input_u8), bool(input_i16)
            self.complex_in = True
        elif kind == "spectrum":
            hop, group, reduce, unit, floor_db = spectrum_args
            check(lib.sdrhip_pipe_spectrum(C.byref(self.h), desc.h, int(hop), int(group), int(reduce), int(unit), float(floor_db)),
                  "sdrhip_pipe_spectrum")
            self.input_u8, self.input_i16 = desc.input_format == IQ_U8, desc.input_format == IQ_I16
            self.complex_in = True
        elif kind == "fm_demod":
            check(lib.sdrhip_pipe_fm_demod(C.byref(self.h)), "sdrhip_pipe_fm_demod")
        elif kind == "am_demod":
            check(lib.sdrhip_pipe_am_demod(C.byref(self.h)), "sdrhip_pipe_am_demod")
        elif kind == "dc_blocker":
            check(lib.sdrhip_pipe_dc_blocker(C.byref(self.h)), "sdrhip_pipe_dc_blocker")
        elif kind == "deemph":
            check(lib.sdrhip_pipe_deemph(C.byref(self.h), mu), "sdrhip_pipe_deemph")
        elif kind == "agc":
            if mu is None or reference is None:
                raise ValueError("Pipe('agc') needs mu and reference")
            check(lib.sdrhip_pipe_agc(C.byref(self.h), mu, reference), "sdrhip_pipe_agc")
        else:
            raise ValueError(kind)
        self.kind = kind

    @staticmethod
    def tuner(tuner, block_size_out):
        """The tuner on host blocks: cfloat blocks in, blocks of block_size_out decimated samples out."""
        return Pipe("tuner", tuner, block_size_out)

    @staticmethod
    def tuner_bank(bank, block_size_out, input_u8=False, input_i16=False):
        """The tuner bank on host blocks: cfloat blocks (or interleaved u8 IQ blocks, input_u8=True, or interleaved int16 IQ blocks,
        input_i16=True; the two exclude each other) in, every channel's blocks of block_size_out decimated samples out."""
        return Pipe("tuner_bank", bank, block_size_out, input_u8=input_u8, input_i16=input_i16)

    @staticmethod
    def am_bank(am_bank, block_size_out, input_u8=False, input_i16=False):
        """The AM bank on host blocks: cfloat, u8 IQ or int16 IQ blocks in, every channel's audio (the envelope; with the bank's
        dc_block, dcBlocker of it, its state kept on the device) in blocks of block_size_out floats out."""
        return Pipe("am_bank", am_bank, block_size_out, input_u8=input_u8, input_i16=input_i16)

    @staticmethod
    def nfm_bank(nfm_bank, block_size_out, input_u8=False, input_i16=False):
        """The narrow-band FM bank on host blocks: cfloat, u8 IQ or int16 IQ blocks in, every channel's fmDemod output (started from
        (0, 0), its state kept on the device) in blocks of block_size_out floats out."""
        return Pipe("nfm_bank", nfm_bank, block_size_out, input_u8=input_u8, input_i16=input_i16)

    @staticmethod
    def am_bank_audio(am_bank, tail, input_u8=False, input_i16=False):
        """The AM bank and its audio stages on host blocks: IQ blocks in, every channel's audio -- Pipe.am_bank's blocks >->
        firResampler >-> firFilter >-> (* gain), all with the AudioTail's block -- in blocks of tail.block floats out."""
        return Pipe("am_bank_audio", (am_bank, tail), tail.block, input_u8=input_u8, input_i16=input_i16)

    @staticmethod
    def narrow_bank(narrow_bank, block_mid, block_size_out, input_u8=False, input_i16=False):
        """The narrow-channel bank on host blocks: IQ blocks in, every channel's  firDecimator deci1 block_mid >-> firDecimator deci2
        block_size_out >-> magnitude | fmDemod [>-> dcBlockingFilter]  in blocks of block_size_out floats out (sdr_hip.h,
        sdrhip_pipe_narrow_bank).  The NarrowBank is borrowed: the pipe keeps a reference to it."""
        return Pipe("narrow_bank", (narrow_bank, block_mid), block_size_out, input_u8=input_u8, input_i16=input_i16)

    @staticmethod
    def narrow_bank_audio(narrow_bank, tail, block_mid, input_u8=False, input_i16=False):
        """The narrow-channel bank and its audio stages on host blocks: IQ blocks in, every channel's audio -- Pipe.narrow_bank's blocks
        >-> firResampler >-> firFilter >-> (* gain), all with the AudioTail's block -- in blocks of tail.block floats out
        (sdrhip_pipe_narrow_bank_audio).  The NarrowBank and the AudioTail are borrowed: the pipe keeps references to them."""
        return Pipe("narrow_bank_audio", (narrow_bank, tail, block_mid), tail.block, input_u8=input_u8, input_i16=input_i16)

    @staticmethod
    def nfm_bank_audio(nfm_bank, tail, input_u8=False, input_i16=False):
        """The narrow-band FM bank and its audio stages on host blocks: as Pipe.am_bank_audio behind Pipe.nfm_bank."""
        return Pipe("nfm_bank_audio", (nfm_bank, tail), tail.block, input_u8=input_u8, input_i16=input_i16)

    @staticmethod
    def spectrum(spectrum, hop=None, group=1, reduce=REDUCE_MEAN_MAGNITUDE, unit=UNIT_LINEAR, floor_db=-200.0):
        """The waterfall on host blocks (sdrhip_pipe_spectrum): blocks of any size in the Spectrum's own input type in (uint8, float32 or
        int16 arrays; an array of another dtype is refused), rows of n float32 out -- output row R reducing input rows R*group ..
        R*group+group-1 of the whole stream, as Spectrum.reduce_device over the concatenated pushes.  hop defaults to n."""
        return Pipe("spectrum", spectrum, spectrum.n, spectrum_args=(spectrum.n if hop is None else hop, group, reduce, unit, floor_db))

    @staticmethod
    def deemph(alpha):
        """De-emphasis on host blocks (sdrhip_pipe_deemph): float32 blocks in, blocks of the same length out, the state (starting at 0)
        carried on the device."""
        return Pipe("deemph", mu=alpha)

    @staticmethod
    def am_demod():
        """The AM envelope detector on host blocks: interleaved complex float32 blocks in, float blocks of the same length out."""
        return Pipe("am_demod")

    @property
    def rows(self):
        """The bank's channel count for Pipe.tuner_bank, 1 for every other pipe."""
        return check(lib.sdrhip_pipe_rows(self.h), "sdrhip_pipe_rows")

    def pop_rows(self, max_blocks):
        """Up to max_blocks blocks of every row at once: an array [rows, nb, floats per block] (sdrhip_pipe_pop_rows)."""
        rows, n = self.rows, self.block_size_out * (2 if self.complex_out else 1)
        o = np.empty((rows, max(max_blocks, 0) * n), np.float32)
        nb = check(lib.sdrhip_pipe_pop_rows(self.h, _fp(o), o.shape[1], max_blocks), "sdrhip_pipe_pop_rows")
        return o[:, : nb * n].reshape(rows, nb, n)

    def _wrong_dtype(self, block, call):
        """A u8 pipe takes uint8 arrays and every other pipe no uint8 array: converting silently would feed the wrong stream."""
        if self.input_i16:
            if getattr(block, "dtype", None) != np.int16:
                raise SdrHipError(f"{call}: this pipe takes int16 IQ blocks, not {getattr(block, 'dtype', type(block).__name__)}")
            return
        is_u8 = getattr(block, "dtype", None) == np.uint8
        if getattr(block, "dtype", None) == np.int16:
            raise SdrHipError(f"{call}: this pipe takes {'uint8 IQ' if self.input_u8 else 'float32'} blocks, not int16")
        if is_u8 != self.input_u8:
            raise SdrHipError(f"{call}: this pipe takes {'uint8 IQ' if self.input_u8 else 'float32'} blocks, not "
                              f"{getattr(block, 'dtype', type(block).__name__)}")

    def push(self, block):
        """block: float32 array (interleaved for complex stages; uint8 IQ for a u8 pipe).  Returns list of output blocks."""
        self._wrong_dtype(block, "Pipe.push")
        if self.input_u8:
            b = np.ascontiguousarray(block, dtype=np.uint8).reshape(-1)
            return self._pop(check(lib.sdrhip_pipe_push_u8(self.h, b.ctypes.data_as(_u8p), b.size // 2), "sdrhip_pipe_push_u8"))
        if self.input_i16:
            b = np.ascontiguousarray(block, dtype=np.int16).reshape(-1)
            return self._pop(check(lib.sdrhip_pipe_push_i16(self.h, b.ctypes.data_as(_i16p), b.size // 2), "sdrhip_pipe_push_i16"))
        b = _f32(block)
        n = b.size // (2 if self.complex_in else 1)
        self._cap = max(getattr(self, "_cap", 0), self.block_size_out, n)
        ready = check(lib.sdrhip_pipe_push(self.h, _fp(b), n), "sdrhip_pipe_push")
        return self._pop(ready)

    def set_coalesce(self, blocks):
        check(lib.sdrhip_pipe_set_coalesce(self.h, blocks), "sdrhip_pipe_set_coalesce")

    def set_adaptive(self, max_blocks):
        check(lib.sdrhip_pipe_set_adaptive(self.h, max_blocks), "sdrhip_pipe_set_adaptive")

    def input_buffer(self, n):
        """numpy view (n elements; interleaved pairs for complex stages) of the pinned staging memory of the next push."""
        fn = lib.sdrhip_pipe_input_buffer_i16 if self.input_i16 else lib.sdrhip_pipe_input_buffer_u8 if self.input_u8 else lib.sdrhip_pipe_input_buffer
        ptr = fn(self.h, n)
        if not ptr:
            raise SdrHipError(lib.sdrhip_last_error().decode())
        if self.input_i16:
            return np.ctypeslib.as_array(C.cast(ptr, _i16p), shape=(2 * n,))
        if self.input_u8:
            return np.ctypeslib.as_array(C.cast(ptr, _u8p), shape=(2 * n,))
        return np.ctypeslib.as_array(C.cast(ptr, _f32p), shape=(n * (2 if self.complex_in else 1),))

    def flush(self):
        ready = check(lib.sdrhip_pipe_flush(self.h), "sdrhip_pipe_flush")
        return self._pop(ready)

    def poll(self):
        """blocks the GPU has finished meanwhile (never waits)"""
        return self._pop(check(lib.sdrhip_pipe_poll(self.h), "sdrhip_pipe_poll"))

    def save(self):
        """sdrhip_pipe_save: drains the pipe and returns its state as bytes (blocks that became ready stay poppable)."""
        lib.sdrhip_pipe_state_bytes.restype = C.c_size_t
        lib.sdrhip_pipe_state_bytes.argtypes = [C.c_void_p]
        cap = lib.sdrhip_pipe_state_bytes(self.h)
        buf = (C.c_ubyte * cap)()
        used = C.c_size_t()
        lib.sdrhip_pipe_save.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        check(lib.sdrhip_pipe_save(self.h, buf, cap, C.byref(used)), "sdrhip_pipe_save")
        return bytes(buf[: used.value])

    def restore(self, state, max_block=0):
        """max_block: fmDemod / dcBlockingFilter pipes hand blocks back at the length they came in; the longest one still
        pending in the state (this wrapper sizes its pop buffer by the longest block it has seen pushed)."""
        lib.sdrhip_pipe_restore.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        self._cap = max(getattr(self, "_cap", 0), int(max_block))
        return self._pop(check(lib.sdrhip_pipe_restore(self.h, state, len(state)), "sdrhip_pipe_restore"))

    def _pop(self, ready):
        if self.kind in ("tuner_bank", "am_bank", "nfm_bank", "am_bank_audio", "nfm_bank_audio", "narrow_bank", "narrow_bank_audio"):
            if ready <= 0:
                return []
            got = self.pop_rows(ready)
            return [np.ascontiguousarray(got[:, k]) for k in range(got.shape[1])]
        outs = []
        cap = max(getattr(self, "_cap", 0), self.block_size_out) * (2 if self.complex_out else 1)
        for _ in range(ready):
            o = np.empty(cap, np.float32)
            got = check(lib.sdrhip_pipe_pop(self.h, _fp(o), cap // (2 if self.complex_out else 1)), "sdrhip_pipe_pop")
            outs.append(o[: got * (2 if self.complex_out else 1)].copy())
        return outs


# Operator-surface aliases with the reference's names (SDR.Filter / SDR.Demod / SDR.Util)
def firFilter(filt, block_size_out):
    return Pipe("filter", filt, block_size_out)


def firDecimator(decimator, block_size_out):
    return Pipe("decimator", decimator, block_size_out)


def firResampler(resampler, block_size_out):
    return Pipe("resampler", resampler, block_size_out)


def fmDemod():
    return Pipe("fm_demod")


def amDemod():
    """`P.map (VG.map magnitude)`: the AM receiver's envelope detector."""
    return Pipe("am_demod")


def dcBlockingFilter():
    """Filter.hs:730-739."""
    return Pipe("dc_blocker")


def agcPipe(mu, reference):
    """Util.hs:344-348: interleaved float32 complex blocks in and out, the state starts at 1."""
    return Pipe("agc", mu=mu, reference=reference)


def interleavedIQUnsignedByteToFloat(u8):
    """Util.hs:104-110: u8 IQ -> complex64 (length len/2)."""
    return DropIn.convert("convertC", u8).view(np.complex64)


def interleavedIQUnsignedByteToFloatFast(u8):
    """Util.hs:137-138 (featureSelect -> AVX2 variant)."""
    return DropIn.convert("convertCAVX", u8).view(np.complex64)
