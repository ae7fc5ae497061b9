"""ctypes binding of libmfa_hip.so (the C ABI declared in include/mfa_hip.h).

The product path has no CPU fallback: if the shared library is missing or cannot be loaded this module raises —
nothing in this package imports the oracle.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

_PKG = Path(__file__).resolve().parent
_SO = Path(os.environ["MFA_HIP_SO"]).resolve() if os.environ.get("MFA_HIP_SO") else _PKG / "libmfa_hip.so"   # (override: A/B builds)
_SOURCES = ["api.hip", "mfcc.hip", "feats.hip", "gmm.hip", "gmm_band.hip", "gmm_pack.cpp", "score_plan.cpp", "viterbi.hip", "viterbi_general.hip",
            "fmllr.hip", "gmm_acc.hip", "gmm_acc_host.cpp", "resample.hip", "resample_plan.cpp", "pitch.hip", "pitch_plan.cpp", "compress.hip", "align_equal.hip", "align_equal_host.cpp",
            "lda_acc.hip", "lda_acc_host.cpp", "mllt_acc.hip", "mllt_acc_host.cpp", "tree_acc.hip", "tree_acc_host.cpp", "vad.hip", "vad_host.cpp", "ubm.hip", "ubm_host.cpp",
            "ivector.hip", "ivector_host.cpp", "plda.hip", "plda_host.cpp", "cluster.hip", "cluster_host.cpp", "hdbscan.hip", "hdbscan_host.cpp",
            "silhouette.hip", "silhouette_host.cpp"]
_LIB = None


class MfaHipError(RuntimeError):
    pass


# d_status codes beyond 0 / 1 (include/mfa_hip.h), as the failure reasons the host layers report
STATUS_REASONS = {
    2: "no alignment within the retry beam",
    3: "token capacity exceeded (device decoder status 3)",
    4: "back-pointer capacity exceeded (device decoder status 4)",
    5: "unsupported graph: a state with more than 64 arcs of a kind (device decoder status 5)",
    6: "internal consistency check failed (device decoder status 6)",
    7: "the best path carries more word labels than the utterance has frames: output labels on epsilon arcs (device decoder status 7)",
}


def status_reason(code: int) -> str:
    return STATUS_REASONS.get(int(code), f"device decoder status {int(code)} (include/mfa_hip.h)")


class MfccOpts(C.Structure):
    _fields_ = [
        ("sample_frequency", C.c_float), ("frame_length_ms", C.c_float), ("frame_shift_ms", C.c_float),
        ("preemphasis", C.c_float), ("low_frequency", C.c_float), ("high_frequency", C.c_float),
        ("cepstral_lifter", C.c_float), ("energy_floor", C.c_float),
        ("num_mel_bins", C.c_int32), ("num_coefficients", C.c_int32), ("snip_edges", C.c_int32),
        ("remove_dc_offset", C.c_int32), ("use_energy", C.c_int32), ("raw_energy", C.c_int32),
    ]


class PitchOpts(C.Structure):
    _fields_ = [
        ("sample_frequency", C.c_float), ("frame_length_ms", C.c_float), ("frame_shift_ms", C.c_float),
        ("min_f0", C.c_float), ("max_f0", C.c_float), ("soft_min_f0", C.c_float), ("penalty_factor", C.c_float),
        ("lowpass_cutoff", C.c_float), ("resample_frequency", C.c_float), ("delta_pitch", C.c_float),
        ("nccf_ballast", C.c_float), ("preemphasis", C.c_float), ("pov_scale", C.c_float), ("pov_offset", C.c_float),
        ("pitch_scale", C.c_float),
        ("lowpass_filter_width", C.c_int32), ("upsample_filter_width", C.c_int32), ("snip_edges", C.c_int32),
        ("normalization_context", C.c_int32), ("add_pov_feature", C.c_int32), ("add_normalized_log_pitch", C.c_int32),
        ("add_raw_log_pitch", C.c_int32), ("add_delta_pitch", C.c_int32),
    ]


class VadOpts(C.Structure):
    _fields_ = [("energy_threshold", C.c_float), ("energy_mean_scale", C.c_float), ("proportion_threshold", C.c_float),
                ("frames_context", C.c_int32)]


class SlidingCmvnOpts(C.Structure):
    _fields_ = [("cmn_window", C.c_int32), ("min_window", C.c_int32), ("center", C.c_int32), ("norm_vars", C.c_int32)]


class GraphBatch(C.Structure):
    _fields_ = [
        ("n_utt", C.c_int32),
        ("d_state_off", C.c_void_p), ("d_arc_base", C.c_void_p), ("d_start", C.c_void_p), ("d_arc_off", C.c_void_p),
        ("d_final", C.c_void_p), ("d_arc_next", C.c_void_p), ("d_arc_weight", C.c_void_p), ("d_arc_col", C.c_void_p),
        ("d_arc_ilabel", C.c_void_p), ("d_arc_olabel", C.c_void_p), ("d_state_nemit", C.c_void_p),
    ]


class ScorePlan(C.Structure):
    _fields_ = [
        ("d_pdf_list", C.c_void_p), ("d_pdf_off", C.c_void_p), ("d_class_counts", C.c_void_p),
        ("d_pdf_first_frame", C.c_void_p), ("d_pdf_last_depth", C.c_void_p), ("d_state_depth", C.c_void_p),
        ("max_cols", C.c_int32), ("groups", C.c_int32), ("d_group_counts", C.c_void_p),
    ]


class AlignOpts(C.Structure):
    _fields_ = [
        ("beam", C.c_float), ("retry_beam", C.c_float), ("acoustic_scale", C.c_float),
        ("max_tokens", C.c_int32), ("bp_tokens_per_frame", C.c_int32),
    ]


def options(struct, defaults: dict, given: dict, what: str, alias: dict = {}):
    """``struct`` filled from ``defaults`` with ``given`` laid over them: a name that is no option is refused (KeyError),
    the integer fields are made integers."""
    d = dict(defaults)
    for k, v in given.items():
        k = alias.get(k, k)
        if k not in d:
            raise KeyError(f"unknown {what} option {k!r}")
        d[k] = v
    return struct(**{k: int(d[k]) if t is C.c_int32 else d[k] for k, t in struct._fields_})


def build_native(force: bool = False, verbose: bool = False) -> Path:
    """Compile the HIP sources for gfx950 into libmfa_hip.so next to this file (hipcc cross-compiles without a GPU)."""
    src_dir = _PKG / "csrc"
    srcs = [src_dir / s for s in _SOURCES]
    headers = ("ctx.hpp", "dev_buf.hpp", "gmm_common.hpp", "gmm_f32.hpp", "gmm_split.hpp", "gmm_pack.hpp", "viterbi_common.hpp", "viterbi_eps.hpp", "viterbi_wave.hpp", "viterbi_small.hpp", "viterbi_plan.hpp",
               "resample_plan.hpp", "pitch_plan.hpp", "compress_math.hpp", "gmm_acc_math.hpp", "gmm_acc_twin.hpp", "acc_posterior.hpp", "acc_segments.hpp", "tid_lookup.hpp", "align_equal_math.hpp", "lda_acc_math.hpp", "mllt_acc_math.hpp", "tree_acc_math.hpp", "vad_math.hpp", "ubm_math.hpp", "ivector_math.hpp", "f64_gemm.hpp", "plda_math.hpp", "cluster_math.hpp", "hdbscan_math.hpp", "pair_sweep.hpp", "silhouette_math.hpp")
    deps = srcs + [src_dir / h for h in headers] + [_PKG.parent / "include" / "mfa_hip.h"]
    if not force and _SO.exists() and all(_SO.stat().st_mtime >= d.stat().st_mtime for d in deps if d.exists()):
        return _SO
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17",
           "-fvisibility=hidden"] + os.environ.get("MFA_HIPCC_FLAGS", "").split() + ["-o", str(_SO)] + [str(s) for s in srcs]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return _SO


# name → (restype, argtypes); mirrors include/mfa_hip.h one to one
_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
SIGNATURES = {
    "mfa_create": (_vp, [C.c_int]),
    "mfa_destroy": (None, [_vp]),
    "mfa_last_error": (C.c_char_p, [_vp]),
    "mfa_version": (C.c_int, []),
    "mfa_set_stream": (C.c_int, [_vp, _vp, C.c_int]),
    "mfa_synchronize": (C.c_int, [_vp]),
    "mfa_device_alloc": (_vp, [_vp, C.c_size_t]),
    "mfa_device_free": (C.c_int, [_vp, _vp]),
    "mfa_memcpy_h2d": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "mfa_memcpy_d2h": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "mfa_timer_begin": (C.c_int, [_vp]),
    "mfa_timer_end_ms": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    "mfa_kernel_timing": (C.c_int, [_vp, C.c_int]),
    "mfa_kernel_time_ms": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "mfa_kernel_time_reset": (C.c_int, [_vp]),
    "mfa_mfcc_configure": (C.c_int, [_vp, C.POINTER(MfccOpts)]),
    "mfa_mfcc_num_frames": (_i32, [_vp, _i64]),
    "mfa_mfcc_batch": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "mfa_mfcc_path": (C.c_int, [_vp]),
    "mfa_gather_pcm": (C.c_int, [_i32, _vp, _vp, _vp, _i32]),
    "mfa_resample_num_samples": (_i64, [_i32, _i32, _i64]),
    "mfa_resample_plan": (C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mfa_resample_plan_general": (C.c_int, [_i32, _i32, C.c_double, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mfa_resample_block_outputs": (_i32, []),
    "mfa_resample_batch": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i64]),
    "mfa_pitch_configure": (C.c_int, [_vp, C.POINTER(PitchOpts)]),
    "mfa_pitch_num_frames": (_i32, [_vp, _i64]),
    "mfa_pitch_num_states": (_i32, [_vp]),
    "mfa_pitch_num_columns": (_i32, [_vp]),
    "mfa_pitch_workspace_bytes": (C.c_size_t, [_vp, _i32, _i64, _i64, _i64, _i32]),
    "mfa_pitch_batch": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "mfa_pitch_process_batch": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32]),
    "mfa_debug_pitch_stages": (C.c_int, [_vp, C.POINTER(PitchOpts), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mfa_cmvn_stats": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _vp]),
    "mfa_feats_batch": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp]),
    "mfa_compress_resident_values": (_i32, []),
    "mfa_compress_batch": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "mfa_debug_compress_host": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mfa_vad_scan_block_frames": (_i32, []),
    "mfa_vad_scan_totals_threads": (_i32, []),
    "mfa_vad_scan_batch": (C.c_int, [_vp, _vp, _vp, _i32, _i64, _vp, _vp]),
    "mfa_debug_vad_scan_host": (C.c_int, [_vp, _vp, _i32, _vp, _vp]),
    "mfa_vad_sum_chunk_frames": (_i32, []),
    "mfa_vad_batch": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i64, _i32, C.POINTER(VadOpts), _vp, _vp, _vp]),
    "mfa_debug_vad_host": (C.c_int, [_vp, _i32, _vp, _i32, C.POINTER(VadOpts), _vp, _vp, _vp]),
    "mfa_sliding_cmvn_tile_frames": (_i32, []),
    "mfa_sliding_cmvn_batch": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, C.POINTER(SlidingCmvnOpts), _vp]),
    "mfa_debug_sliding_cmvn_host": (C.c_int, [_vp, _vp, _i32, _i32, _i32, C.POINTER(SlidingCmvnOpts), _vp]),
    "mfa_select_frames_count": (C.c_int, [_vp, _vp, _vp, _i32, _i64, _i32, _vp, _vp]),
    "mfa_select_frames_batch": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i64, _vp, _i32]),
    "mfa_debug_select_frames_host": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp]),
    "mfa_vad_runs_batch": (C.c_int, [_vp, _vp, _vp, _i32, _i64, _i64, _vp, _vp, _vp]),
    "mfa_debug_vad_runs_host": (C.c_int, [_vp, _vp, _i32, _i64, _vp, _vp, _vp]),
    "mfa_load_gmm": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mfa_gmm_slot": (_i32, [_vp, _i32]),
    "mfa_gmm_sort_pdf_list": (C.c_int, [_vp, _vp, _i32, _vp]),
    "mfa_gmm_sort_pdf_list_keyed": (C.c_int, [_vp, _vp, _vp, _i32, _vp]),
    "mfa_fst_first_frames": (C.c_int, [_i32, _vp, _vp, _i32, _vp]),
    "mfa_debug_gmm_trace": (C.c_int, [_vp, _vp]),
    "mfa_debug_gmm_pack": (C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _i32, _vp]),
    "mfa_debug_viterbi_stamps": (C.c_int, [_vp, _vp]),
    "mfa_debug_viterbi_plan": (C.c_int, [C.POINTER(AlignOpts), _i32, _i32, _i32, _i32, _vp, _i32]),
    "mfa_gmm_score_batch": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mfa_align_batch": (C.c_int, [_vp, C.POINTER(GraphBatch), _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, C.POINTER(AlignOpts),
                                  _vp, _vp, _vp, _vp, _vp, _vp]),
    "mfa_align_general_batch": (C.c_int, [_vp, C.POINTER(GraphBatch), _vp, _vp, _vp, _vp, _vp, _i32, _i32, C.POINTER(AlignOpts),
                                          _vp, _vp, _vp, _vp, _vp, _vp]),
    "mfa_align_features_batch": (C.c_int, [_vp, C.POINTER(GraphBatch), C.POINTER(ScorePlan), _vp, _vp, _i32, _i64, _i64, _i32, _i32,
                                           C.POINTER(AlignOpts), _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mfa_fst_last_depths": (C.c_int, [_i32, _vp, _vp, _i32, _vp, _vp]),
    "mfa_build_score_plan": (C.c_int, [_i32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mfa_build_score_plan_grouped": (C.c_int, [_i32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mfa_build_score_plans_batch": (C.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp,
                                              _vp, _vp, _vp, _vp, _vp]),
    "mfa_fmllr_acc_batch": (C.c_int, [_vp, _vp, _vp, _i32, _i64, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "mfa_fmllr_acc_ali_batch": (C.c_int, [_vp, _vp, _vp, _i32, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "mfa_fmllr_stats_model": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp]),
    "mfa_gmm_acc_chunk_frames": (_i32, []),
    "mfa_gmm_acc_max_dim": (_i32, []),
    "mfa_gmm_acc_batch": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mfa_debug_gmm_acc_host": (C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _i32]),
    "mfa_gmm_acc_twofeats_batch": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mfa_debug_gmm_acc_twofeats_host": (C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp,
                                                   _vp, _vp, _vp, _i32]),
    "mfa_align_equal_batch": (C.c_int, [_vp, C.POINTER(GraphBatch), _vp, _i64, _i64, _vp, C.c_uint32, _vp, _vp]),
    "mfa_debug_align_equal_host": (C.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp]),
    "mfa_lda_acc_slab_frames": (_i32, []),
    "mfa_lda_acc_chunk_frames": (_i32, []),
    "mfa_lda_acc_max_dim": (_i32, []),
    "mfa_lda_acc_batch": (C.c_int, [_vp, _vp, _vp, _i32, _i64, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _f32, _vp, C.c_uint32,
                                    _vp, _vp, _vp, _vp]),
    "mfa_debug_lda_acc_host": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _f32, _vp, C.c_uint32,
                                         _vp, _vp, _vp, _vp]),
    "mfa_mllt_acc_chunk_frames": (_i32, []),
    "mfa_mllt_acc_max_dim": (_i32, []),
    "mfa_mllt_acc_batch": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "mfa_debug_mllt_acc_host": (C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32]),
    "mfa_tree_acc_chunk_frames": (_i32, []),
    "mfa_tree_acc_max_dim": (_i32, []),
    "mfa_tree_acc_batch": (C.c_int, [_vp, _vp, _vp, _i32, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i64, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _vp]),
    "mfa_debug_tree_acc_host": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i64, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _vp]),
    "mfa_ubm_gselect_batch": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp]),
    "mfa_debug_ubm_gselect_host": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp]),
    "mfa_ubm_acc_slab_frames": (_i32, []),
    "mfa_ubm_gselect_tile_frames": (_i32, []),
    "mfa_ubm_acc_batch": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mfa_debug_ubm_acc_host": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mfa_ivector_prune_post_batch": (C.c_int, [_vp, _vp, _i64, _i32, _f32, _f32, _vp]),
    "mfa_debug_ivector_prune_post_host": (C.c_int, [_vp, _i64, _i32, _f32, _f32, _vp]),
    "mfa_ivector_scatter_slab_frames": (_i32, []),
    "mfa_ivector_utt_stats_batch": (C.c_int, [_vp, _vp, _vp, _i32, _i64, _i32, _i32, _i32, _vp, _vp, C.c_double, _vp, _vp, _vp]),
    "mfa_debug_ivector_utt_stats_host": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, C.c_double, _vp, _vp, _vp]),
    "mfa_ivector_estep_batch": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _vp]),
    "mfa_debug_ivector_estep_host": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                               _vp, _vp]),
    "mfa_plda_transform_batch": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "mfa_debug_plda_transform_host": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "mfa_plda_score_batch": (C.c_int, [_vp, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mfa_debug_plda_score_host": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mfa_debug_plda_prepare_host": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mfa_debug_plda_sweep_batch": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mfa_debug_plda_sweep_host": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mfa_neighbor_bits_batch": (C.c_int, [_vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _i32, _i32, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mfa_debug_neighbor_bits_host": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _i32, _i32, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mfa_debug_neighbor_sweep_batch": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _i32, _i32, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mfa_debug_neighbor_sweep_host": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _i64, _i32, _i32, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mfa_dbscan_from_bits": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, C.POINTER(_i32), C.POINTER(_i32)]),
    "mfa_debug_dbscan_from_bits_host": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, C.POINTER(_i32)]),
    "mfa_hdbscan_core_batch": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    "mfa_hdbscan_mst_batch": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, C.POINTER(_i32), C.POINTER(_i32)]),
    "mfa_debug_hdbscan_core_host": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mfa_debug_hdbscan_mst_host": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, C.POINTER(_i32)]),
    "mfa_silhouette_batch": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mfa_debug_silhouette_host": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mfa_align_workspace_bytes": (C.c_size_t, [_vp, _i32, _i64, C.POINTER(AlignOpts)]),
}


# entry points that builds loaded through MFA_HIP_SO (older ones, for A/B timing) may lack
_NEWER = {"mfa_mfcc_path", "mfa_gmm_acc_twofeats_batch", "mfa_debug_gmm_acc_twofeats_host", "mfa_debug_viterbi_plan"}


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        if not _SO.exists():
            raise MfaHipError(
                f"{_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(the alignment path has no CPU fallback)"
            )
        # torch first: it brings its own HIP runtime, and the process must end up with ONE (device buffers and streams
        # are shared with torch); loading libmfa_hip.so first would bind it to a second copy of libamdhip64
        import torch  # noqa: F401

        try:
            handle = C.CDLL(str(_SO))
        except OSError as e:  # e.g. no ROCm runtime on this machine
            raise MfaHipError(f"cannot load {_SO}: {e}") from e
        for name, (res, args) in SIGNATURES.items():
            if name in _NEWER and os.environ.get("MFA_HIP_SO") and not hasattr(handle, name):
                continue                 # an older build under A/B: calling the entry point raises AttributeError
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = handle
    return _LIB


def check(ctx, rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().mfa_last_error(ctx)
        raise MfaHipError(f"{what}: {msg.decode() if msg else 'error'}")


def twin_check(rc: int, name: str, codes: dict = {}) -> None:
    """The return code of a host twin (no context, so no ``mfa_last_error``): ``codes`` holds its stage's reasons."""
    if rc != 0:
        raise MfaHipError(f"{name}: {codes.get(rc, 'bad arguments')}")


def twin_call(name: str, codes: dict, *args) -> None:
    """Host twin ``name`` of the library on ``args``, the numpy arrays among them as pointers (``_np_ptr``; ``args`` keeps them
    alive across the call), its return code through ``twin_check``."""
    twin_check(getattr(lib(), name)(*(_np_ptr(a) if hasattr(a, "ctypes") else a for a in args)), name, codes)


def _ptr(t):
    """A torch tensor (or None) as the pointer argument of a library call."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _elem_ptr(t, index: int):
    """Element ``index`` of a 1-D torch tensor as the pointer argument of a library call."""
    return C.c_void_p(t.data_ptr() + index * t.element_size())


def _np_ptr(a):
    """A numpy array (or None) as the pointer argument of a library call; the caller keeps it alive across the call."""
    return None if a is None else a.ctypes.data
