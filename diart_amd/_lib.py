"""ctypes binding of ``libdiart_amd.so`` (the C ABI declared in ``include/diart_amd.h``).

There is no CPU fallback: if the shared object is missing or a call fails this module
raises.  ``load()`` does not need a GPU (the CPU test-suite checks that every declared
symbol is exported); creating a context does.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Optional

# DZ_EXPERIMENTS=1 loads the experiments build (`python -m diart_amd.build --experiments`: the never-default
# kernel generations and the DZ_* switches that select them, include/diart_amd_experiments.h)
EXPERIMENTS = os.environ.get("DZ_EXPERIMENTS", "0") not in ("", "0")
_LIB_PATH = Path(__file__).resolve().parent / ("libdiart_amd_exp.so" if EXPERIMENTS else "libdiart_amd.so")
_lib: Optional[C.CDLL] = None

c_float_p = C.POINTER(C.c_float)
c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int)
vp = C.c_void_p


class SincNetWeights(C.Structure):
    _fields_ = [("wav_gamma", C.c_float), ("wav_beta", C.c_float)] + [
        (n, vp) for n in ("filt", "in0_g", "in0_b", "w1", "b1", "in1_g", "in1_b",
                          "w2", "b2", "in2_g", "in2_b", "w1_split", "w2_split", "filt_split")]


class SegWeights(C.Structure):
    _fields_ = [("sinc", SincNetWeights), ("wih", vp * 4), ("bih", vp * 4), ("whh", vp * 4),
                ("lin0_w", vp), ("lin0_b", vp), ("lin1_w", vp), ("lin1_b", vp),
                ("cls_w", vp), ("cls_b", vp),
                ("num_classes", C.c_int), ("powerset", C.c_int), ("num_speakers", C.c_int),
                ("wih_split", vp * 4), ("lin0_split", vp), ("lin1_split", vp), ("whh_split", vp * 4), ("lstm_variant", C.c_int), ("wih0_split_kb", vp)]


class EmbWeights(C.Structure):
    _fields_ = [("sinc", SincNetWeights), ("tw", vp * 5), ("tb", vp * 5), ("ts", vp * 5),
                ("th", vp * 5), ("emb_w", vp), ("emb_b", vp), ("dimension", C.c_int),
                ("tw_split", vp * 5), ("tw0_split_kb", vp), ("pool_nearest", C.c_int)]


TRACK_SPEECH, TRACK_OVERLAP = 0, 1   # DZ_TRACK_*: the track dz_seg_forward_track's head writes beside the scores
GATHER_MAX_RUNS = 64            # DZ_GATHER_MAX_RUNS: runs one launch of dz_gather_windows carries


class WindowRun(C.Structure):   # dz_window_run
    _fields_ = [("src", vp), ("row0", C.c_int), ("count", C.c_int)]


class Layer(C.Structure):
    _fields_ = [("w", vp), ("b", vp), ("s", vp), ("h", vp), ("wsplit", vp)]


class SeRes2Net(C.Structure):
    _fields_ = [("tdnn1", Layer), ("res", Layer * 7), ("tdnn2", Layer), ("se1", Layer), ("se2", Layer)]


class EcapaWeights(C.Structure):
    _fields_ = [("dft", vp), ("mel", vp), ("block0", Layer), ("ser", SeRes2Net * 3), ("mfa", Layer),
                ("asp_tdnn", Layer), ("asp_wms", vp), ("asp_conv", Layer), ("fc", Layer), ("zeros", vp),
                ("dft_split", vp)]


class EcmWeights(C.Structure):
    _fields_ = [("net", EcapaWeights), ("dft", vp), ("dft_split", vp), ("mel", vp), ("min_num_samples", C.c_int)]


class WspConv(C.Structure):
    _fields_ = [("w", vp), ("b", vp), ("wsplit", vp)]


class WspWeights(C.Structure):
    _fields_ = [("mel", vp), ("conv1", WspConv), ("block", (WspConv * 3) * 16), ("seg_w", vp), ("seg_b", vp)]


class SbxWeights(C.Structure):
    _fields_ = [("dft", vp), ("dft_split", vp), ("mel", vp), ("tdnn", Layer * 5), ("lin_w", vp), ("lin_b", vp),
                ("zeros", vp)]


class TtnSep(C.Structure):
    _fields_ = [("dw", vp), ("pw", Layer)]


class TtnBlock(C.Structure):
    _fields_ = [("rep", TtnSep * 3), ("se1", vp), ("se2t", vp), ("res", Layer)]


class TtnWeights(C.Structure):
    _fields_ = [("dft", vp), ("dft_split", vp), ("mel", vp), ("block", TtnBlock * 5), ("asp_tdnn", Layer),
                ("asp_wms", vp), ("asp_conv", Layer), ("fc", Layer), ("zeros", vp), ("pad_reflect", C.c_int),
                ("frame_pad", C.c_int), ("frame_nfft", C.c_int), ("min_num_samples", C.c_int)]


class SbrBlock(C.Structure):
    _fields_ = [("conv", WspConv * 3), ("se_w1t", vp), ("se_b1", vp), ("se_w2t", vp), ("se_b2", vp),
                ("width", C.c_int), ("se_width", C.c_int), ("stride", C.c_int), ("layer", C.c_int)]


SBR_MAX_BLOCKS = 32


class SbrWeights(C.Structure):
    _fields_ = [("dft", vp), ("dft_split", vp), ("mel", vp), ("stem_w", vp), ("stem_b", vp),
                ("block", SbrBlock * SBR_MAX_BLOCKS), ("att1", Layer), ("att2", Layer), ("fc", Layer), ("zeros", vp),
                ("n_blocks", C.c_int), ("stem_width", C.c_int), ("min_num_samples", C.c_int), ("rows_per_pass", C.c_int)]


class TuneDesc(C.Structure):
    _fields_ = [(n, vp) for n in ("seg", "emb", "pre_max", "pre_mean", "pre_flags", "chunk_off", "plan", "row_off",
                                  "row_chunk", "hamming")] + [
        (n, C.c_int) for n in ("N", "F", "K", "D", "G", "nwin", "total_chunks", "total_rows")]


class TuneCells(C.Structure):
    POINTERS = ("file_chunk_off", "file_row_off", "row_off", "step_rows", "mids", "mid_cell", "file_cell_off", "cell_dur",
                "cell_ref", "cell_step", "dur_prefix", "ref_prefix")
    _fields_ = [(n, vp) for n in POINTERS] + [
        (n, C.c_int) for n in ("n_files", "total_rows", "total_chunks", "max_cells", "max_speakers")] + [("collar", C.c_double)]


# name -> (restype, argtypes); must list every function of include/diart_amd.h
SIGNATURES = {
    "dz_last_error": (C.c_char_p, []),
    "dz_version": (C.c_int, []),
    "dz_set_option": (C.c_int, [C.c_char_p, C.c_int]),
    "dz_get_option": (C.c_int, [C.c_char_p, c_int_p]),
    "dz_has_experiments": (C.c_int, []),
    "dz_host_pool_set_spin": (C.c_int, [C.c_int]),
    "dz_abi_struct_sizes": (C.c_int, [C.POINTER(C.c_int * 5)]),
    "dz_ctx_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
    "dz_ctx_destroy": (C.c_int, [vp]),
    "dz_range_check": (C.c_int, [vp, C.c_int]),
    "dz_seg_frames_for": (C.c_int, [C.c_int]),
    "dz_emb_frames_for": (C.c_int, [C.c_int]),
    "dz_seg_create": (C.c_int, [vp, C.POINTER(SegWeights), C.c_int, C.c_int, C.POINTER(vp)]),
    "dz_seg_forward": (C.c_int, [vp, vp, C.c_longlong, C.c_int, vp, vp]),
    "dz_seg_forward_osp": (C.c_int, [vp, vp, C.c_longlong, C.c_int, vp, C.c_float, C.c_float, C.c_int, vp, vp]),
    "dz_seg_forward_vad": (C.c_int, [vp, vp, C.c_longlong, C.c_int, vp, vp, vp]),
    "dz_seg_forward_track": (C.c_int, [vp, vp, C.c_longlong, C.c_int, vp, vp, C.c_int, vp]),
    "dz_overlap_track": (C.c_int, [vp, C.c_longlong, C.c_longlong, C.c_int, vp, vp]),
    "dz_seg_destroy": (C.c_int, [vp]),
    "dz_emb_create": (C.c_int, [vp, C.POINTER(EmbWeights), C.c_int, C.c_int, C.POINTER(vp)]),
    "dz_emb_forward": (C.c_int, [vp, vp, C.c_longlong, vp, C.c_int, C.c_int, vp, vp]),
    "dz_emb_forward_multi": (C.c_int, [vp, vp, C.c_longlong, vp, C.c_int, C.c_int, C.c_int,
                                       C.c_int, vp, vp]),
    "dz_emb_frames": (C.c_int, [vp, vp, C.c_longlong, C.c_int, vp]),
    "dz_seg_front": (C.c_int, [vp, vp, C.c_longlong, C.c_int, vp]),
    "dz_seg_back": (C.c_int, [vp, C.c_int, vp, C.c_float, C.c_float, C.c_int, vp, vp]),
    "dz_wave_stats_floats": (C.c_int, []),
    "dz_wave_stats": (C.c_int, [vp, vp, C.c_longlong, C.c_int, C.c_int, vp, vp]),
    "dz_seg_use_wave_stats": (C.c_int, [vp, vp]),
    "dz_emb_use_wave_stats": (C.c_int, [vp, vp]),
    "dz_emb_pool": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "dz_emb_peek": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "dz_emb_destroy": (C.c_int, [vp]),
    "dz_ecapa_frames_for": (C.c_int, [C.c_int]),
    "dz_ecapa_create": (C.c_int, [vp, C.POINTER(EcapaWeights), C.c_int, C.c_int, C.POINTER(vp)]),
    "dz_ecapa_forward": (C.c_int, [vp, vp, C.c_longlong, vp, C.c_int, C.c_int, vp, vp]),
    "dz_ecapa_forward_groups": (C.c_int, [vp, vp, C.c_longlong, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "dz_ecapa_peek": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "dz_ecapa_destroy": (C.c_int, [vp]),
    "dz_ecm_abi_size": (C.c_int, []),
    "dz_ecm_frames_for": (C.c_int, [C.c_int]),
    "dz_ecm_create": (C.c_int, [vp, C.POINTER(EcmWeights), C.c_int, C.c_int, C.POINTER(vp)]),
    "dz_ecm_forward": (C.c_int, [vp, vp, C.c_longlong, vp, C.c_int, C.c_int, vp, vp]),
    "dz_ecm_forward_groups": (C.c_int, [vp, vp, C.c_longlong, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "dz_ecm_peek": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "dz_ecm_destroy": (C.c_int, [vp]),
    "dz_sbx_abi_size": (C.c_int, []),
    "dz_sbx_create": (C.c_int, [vp, C.POINTER(SbxWeights), C.c_int, C.c_int, C.POINTER(vp)]),
    "dz_sbx_forward": (C.c_int, [vp, vp, C.c_longlong, vp, C.c_int, C.c_int, vp, vp]),
    "dz_sbx_forward_groups": (C.c_int, [vp, vp, C.c_longlong, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "dz_sbx_peek": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "dz_sbx_destroy": (C.c_int, [vp]),
    "dz_ttn_abi_size": (C.c_int, []),
    "dz_ttn_frames_for": (C.c_int, [C.c_int]),
    "dz_ttn_create": (C.c_int, [vp, C.POINTER(TtnWeights), C.c_int, C.c_int, C.POINTER(vp)]),
    "dz_ttn_forward": (C.c_int, [vp, vp, C.c_longlong, vp, C.c_int, C.c_int, vp, vp]),
    "dz_ttn_forward_groups": (C.c_int, [vp, vp, C.c_longlong, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "dz_ttn_peek": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "dz_ttn_destroy": (C.c_int, [vp]),
    "dz_sbr_abi_size": (C.c_int, []),
    "dz_sbr_create": (C.c_int, [vp, C.POINTER(SbrWeights), C.c_int, C.c_int, C.POINTER(vp)]),
    "dz_sbr_forward": (C.c_int, [vp, vp, C.c_longlong, vp, C.c_int, C.c_int, vp, vp]),
    "dz_sbr_forward_groups": (C.c_int, [vp, vp, C.c_longlong, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "dz_sbr_peek": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "dz_sbr_destroy": (C.c_int, [vp]),
    "dz_wsp_abi_size": (C.c_int, []),
    "dz_wsp_frames_for": (C.c_int, [C.c_int, C.c_int]),
    "dz_wsp_create": (C.c_int, [vp, C.POINTER(WspWeights), C.c_int, C.c_int, C.POINTER(vp)]),
    "dz_wsp_forward": (C.c_int, [vp, vp, C.c_longlong, vp, C.c_int, C.c_int, vp, vp]),
    "dz_wsp_forward_multi": (C.c_int, [vp, vp, C.c_longlong, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "dz_wsp_trunk": (C.c_int, [vp, vp, C.c_longlong, C.c_int, vp]),
    "dz_wsp_pool": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "dz_wsp_peek": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "dz_wsp_destroy": (C.c_int, [vp]),
    "dz_resample_geometry": (C.c_int, [C.c_int, C.c_int, c_int_p, c_int_p, c_int_p, c_int_p]),
    "dz_resample_out_len": (C.c_longlong, [C.c_int, C.c_int, C.c_longlong]),
    "dz_resample_table": (C.c_int, [C.c_int, C.c_int, c_float_p]),
    "dz_resample_create": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(vp)]),
    "dz_resample_forward": (C.c_int, [vp, vp, C.c_longlong, C.c_longlong, C.c_int, vp, C.c_longlong, vp]),
    "dz_resample_destroy": (C.c_int, [vp]),
    "dz_adjust_volume": (C.c_int, [vp, vp, C.c_longlong, vp, C.c_longlong, C.c_int, C.c_longlong, C.c_int, C.c_double,
                                   vp]),
    "dz_prof_enable": (C.c_int, [C.c_int]),
    "dz_prof_pause": (C.c_int, [C.c_int]),
    "dz_prof_collect": (C.c_int, []),
    "dz_prof_get": (C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_double),
                              C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "dz_osp": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int,
                         C.c_int, vp, vp]),
    "dz_l2_normalize": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_float, vp]),
    "dz_results_to_host": (C.c_int, [vp, vp, vp, C.c_longlong, vp, vp, C.c_longlong, vp]),
    "dz_cdist_cosine": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "dz_clu_create": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_int, C.POINTER(vp)]),
    "dz_clu_reset": (C.c_int, [vp]),
    "dz_clu_step": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp]),
    "dz_clu_step_batch": (C.c_int, [C.POINTER(vp), C.c_int, vp, C.c_int, C.c_int, vp, C.c_int,
                                    vp, vp, C.c_int]),
    "dz_clu_get_centers": (C.c_int, [vp, vp, C.c_int]),
    "dz_clu_get_active": (C.c_int, [vp, vp]),
    "dz_clu_dim": (C.c_int, [vp]),
    "dz_clu_set_state": (C.c_int, [vp, vp, vp, C.c_int]),
    "dz_clu_destroy": (C.c_int, [vp]),
    "dz_lsap": (C.c_int, [vp, C.c_int, C.c_int, vp]),
    "dz_ring_create": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "dz_ring_reset": (C.c_int, [vp]),
    "dz_ring_destroy": (C.c_int, [vp]),
    "dz_ring_push": (C.c_int, [vp, vp, C.c_longlong, C.c_int, vp]),
    "dz_ring_window": (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "dz_ring_read": (C.c_int, [vp, vp, vp]),
    "dz_ring_push_rows": (C.c_int, [vp, vp, C.c_longlong, C.c_int, C.POINTER(C.c_int), C.c_int, vp]),
    "dz_ring_push_rows_pcm": (C.c_int, [vp, vp, C.c_longlong, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, vp]),
    "dz_pcm_decode": (C.c_int, [vp, vp, C.c_longlong, C.c_int, C.c_int, vp, vp]),
    "dz_ring_filled_row": (C.c_int, [vp, C.c_int, C.POINTER(C.c_int)]),
    "dz_ring_gather": (C.c_int, [vp, C.POINTER(C.c_int), C.c_int, vp, C.c_longlong, vp]),
    "dz_ring_reset_row": (C.c_int, [vp, C.c_int]),
    "dz_tail_create": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int,
                                 C.c_int, vp, C.POINTER(vp)]),
    "dz_tail_reset": (C.c_int, [vp]),
    "dz_tail_set_offset": (C.c_int, [vp, C.c_double]),
    "dz_tail_destroy": (C.c_int, [vp]),
    "dz_tail_max_rows": (C.c_int, [vp]),
    "dz_tail_speakers": (C.c_int, [vp]),
    "dz_tail_step": (C.c_int, [vp, vp, C.c_double, C.c_double, vp, vp, vp, vp, vp, C.c_int, vp]),
    "dz_tail_step_batch": (C.c_int, [C.POINTER(vp), C.c_int, vp, vp, vp, vp, vp, vp, vp, vp,
                                     C.c_int, vp, C.c_int]),
    "dz_file_step_batch": (C.c_int, [C.POINTER(vp), C.POINTER(vp), C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int,
                                     C.c_int, vp, C.c_double, vp, C.c_int, vp, vp, C.c_int]),
    "dz_file_vad_step_batch": (C.c_int, [C.POINTER(vp), C.c_int, vp, vp, vp, C.c_int, vp, C.c_double, vp, C.c_int, vp,
                                         C.c_int]),
    "dz_gather_windows": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_longlong, C.c_int, vp]),
    "dz_tune_abi_size": (C.c_int, []),
    "dz_tune_plan": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_double, vp, vp, vp, vp, vp]),
    "dz_tune_replay": (C.c_int, [vp, C.POINTER(TuneDesc), vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, vp]),
    "dz_tune_replay_host": (C.c_int, [C.POINTER(TuneDesc), vp, C.c_int, C.c_double, C.c_double, vp, vp, vp, vp, vp,
                                      C.c_int, C.c_int]),
    "dz_tune_cells_abi_size": (C.c_int, []),
    "dz_tune_score": (C.c_int, [C.POINTER(TuneCells), C.c_int, vp, vp, C.c_int]),
    "dz_tune_score_gpu": (C.c_int, [vp, C.POINTER(TuneCells), C.c_int, vp, vp, vp, C.c_int, vp, vp]),
    "dz_tune_score_core": (C.c_int, [C.POINTER(TuneCells), C.c_int, vp, C.c_int, C.c_int, vp, C.c_int]),
    "dz_tune_vad_rows": (C.c_int, [vp, C.POINTER(TuneDesc), vp, vp]),
    "dz_tune_vad_score": (C.c_int, [vp, C.POINTER(TuneCells), C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]),
    "dz_tune_vad_host": (C.c_int, [C.POINTER(TuneDesc), C.POINTER(TuneCells), C.c_int, vp, C.c_int, vp, vp, C.c_int, vp,
                                   C.c_int]),
    "dz_tune_track_score_dur": (C.c_int, [C.POINTER(TuneCells), C.c_int, vp, vp, vp, C.c_int]),
    "dz_tune_vad_replay_tails": (C.c_int, [C.POINTER(TuneDesc), vp, C.c_int, C.c_double, C.c_double, vp, vp, vp, C.c_int]),
    # (the naming entries score nothing and take no dz_tune_cells: their arrays are a trial's, loose as in the header)
    "dz_tune_name": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp,
                               vp, vp, vp, vp, C.c_int, vp]),
    "dz_tune_name_host": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp,
                                    vp, vp, vp, vp, C.c_int]),
    "dz_tune_ident_score": (C.c_int, [C.POINTER(TuneCells), C.c_int, vp, vp, vp, C.c_int]),
    "dz_tune_ident_score_gpu": (C.c_int, [vp, C.POINTER(TuneCells), C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp]),
    "dz_tune_ident_score_core": (C.c_int, [C.POINTER(TuneCells), C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int]),
    "dz_agglo_work_bytes": (C.c_longlong, [C.c_int, vp]),
    "dz_agglo_linkage": (C.c_int, [vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_longlong, vp]),
    "dz_agglo_linkage_host": (C.c_int, [C.c_int, vp, vp, C.c_int, vp, vp, C.c_int]),
    "dz_agglo_cut": (C.c_int, [vp, C.c_int, C.c_double, C.c_int, C.c_int, vp, c_int_p]),
    "dz_offline_assign": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp]),
    "dz_offline_reconstruct": (C.c_int, [C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_double, vp, vp, C.c_int]),
    "dz_rows_repeat": (C.c_int, [vp, vp, C.c_longlong, C.c_int, C.c_int, vp, c_int_p]),
    "dz_gallery_create": (C.c_int, [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]),
    "dz_gallery_destroy": (C.c_int, [vp]),
    "dz_gallery_size": (C.c_int, [vp]),
    "dz_gallery_dim": (C.c_int, [vp]),
    "dz_gallery_match": (C.c_int, [vp, vp, C.c_longlong, C.c_int, vp, vp, vp, vp]),
    "dz_gallery_set_cohort": (C.c_int, [vp, vp, C.c_int, C.c_int]),
    "dz_gallery_cohort_size": (C.c_int, [vp]),
    "dz_gallery_cohort_stats": (C.c_int, [vp, vp, C.c_longlong, C.c_int, vp, vp, vp]),
    "dz_gallery_entry_stats": (C.c_int, [vp, vp, vp]),
    "dz_gallery_match_norm": (C.c_int, [vp, vp, C.c_longlong, C.c_int, vp, vp, vp, vp]),
    # kernel-level entry points
    "dz_k_convgemm": (C.c_int, [vp, vp, vp]),
    "dz_k_gemm_f32": (C.c_int, [vp, vp, vp]),
    "dz_k_gemm_split": (C.c_int, [vp, vp, vp]),
    "dz_k_gemm_pre": (C.c_int, [vp, vp, vp]),
    "dz_k_mlp_head": (C.c_int, [vp, vp, C.c_longlong, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_int, C.c_float, C.c_float, vp, vp, vp]),
    "dz_k_seg_head": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_float,
                                C.c_float, C.c_int, vp, vp]),
    "dz_k_conv_pool": (C.c_int, [vp, vp, vp]),
    "dz_k_convgemm_ntile": (C.c_int, [C.c_int]),
    "dz_k_wave_stats": (C.c_int, [vp, vp, C.c_longlong, C.c_int, C.c_int, vp, vp]),
    "dz_k_sinc_conv0": (C.c_int, [vp, vp, C.c_longlong, C.c_int, C.c_int, vp, C.c_float,
                                  C.c_float, vp, vp, vp, vp]),
    "dz_k_sinc_conv0_split": (C.c_int, [vp, vp, C.c_longlong, C.c_int, C.c_int, vp, C.c_float,
                                        C.c_float, vp, vp, vp, vp]),
    "dz_k_conv0_split_ntile": (C.c_int, [C.c_int]),
    "dz_k_finalize_norm": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]),
    "dz_k_lstm": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, vp]),
    "dz_k_lstm_mfma": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "dz_k_lstm_planes": (C.c_int, [vp, vp, vp, vp, C.c_int, vp, C.c_longlong, C.c_int, C.c_int, vp]),
    "dz_k_stats_pool": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int,
                                  C.c_int, vp, C.c_int, vp]),
    "dz_k_pool_pieces": (C.c_int, [C.c_int]),
    "dz_k_tdnn_pool": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp,
                                 C.c_int, vp]),
    "dz_k_powerset": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "dz_k_conv2d": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                              C.c_int, C.c_int, vp]),
    "dz_k_conv2d_masked": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, vp]),
    "dz_k_sbr_se_gate": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]),
    "dz_k_sbr_se_apply": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "dz_k_sbr_att_pool": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "dz_k_ttn_depthwise": (C.c_int, [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
}


# include/diart_amd_experiments.h: bound only when the loaded library is the experiments build
EXPERIMENT_SIGNATURES = {
    "dz_k_gemm_g2": (C.c_int, [vp, vp, C.c_int, vp]),
    "dz_k_gemm_g3": (C.c_int, [vp, vp, C.c_int, vp]),
    "dz_k_conv_pool_debug": (C.c_int, [vp]),
    "dz_sinc_conv0_pair": (C.c_int, [vp, vp, vp, C.c_longlong, C.c_int, vp, vp, vp, vp]),
    "dz_k_sinc_conv0_pair": (C.c_int, [vp, vp, C.c_longlong, C.c_int, C.c_int, vp, vp, vp, C.c_float, C.c_float, vp, vp,
                                       vp, vp, vp]),
}


class ConvGemmDesc(C.Structure):
    _fields_ = [(n, vp) for n in ("X", "W", "bias", "e0", "e1", "nscale", "nshift", "Y", "partials")] + [
        (n, C.c_int) for n in ("B", "Tin", "Tout", "Cin", "taps", "dil", "K", "Kpad", "Npad",
                               "Nstore", "ldx", "ldy", "nld", "Tstore")] + [
        ("xbs", C.c_longlong), ("ybs", C.c_longlong), ("norm_on_load", C.c_int), ("epi", C.c_int),
        ("ksplit", C.c_int), ("ysplit", C.c_longlong), ("agroup", C.c_int), ("pad", C.c_int),
        ("X2", vp), ("rowbias", vp), ("Wsplit", vp), ("Xsplit", vp), ("xplane", C.c_longlong),
        ("Ysplit", vp), ("yplane", C.c_longlong), ("npart", vp), ("ngamma", vp), ("nbeta", vp),
        ("npart_tiles", C.c_int), ("npart_T", C.c_int), ("oflag", vp), ("Tdev", vp)]


(EPI_BIAS, EPI_BIAS_LEAKY, EPI_BIAS_SIGMOID, EPI_TDNN, EPI_POOL3, EPI_BIAS_RELU, EPI_RELU_BN,
 EPI_RELU_BN_TANH) = range(8)


class DiartAmdError(RuntimeError):
    pass


def lib_path() -> Path:
    return _LIB_PATH


def load() -> C.CDLL:
    """dlopen the library and attach prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not _LIB_PATH.exists():
            raise DiartAmdError(
                f"{_LIB_PATH} not found: build it with `python -m diart_amd.build` "
                "(hipcc, gfx950).  diart_amd has no CPU fallback.")
        lib = C.CDLL(str(_LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if a declared symbol is missing
            fn.restype = res
            fn.argtypes = args
        if lib.dz_has_experiments():
            for name, (res, args) in EXPERIMENT_SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
        elif EXPERIMENTS:
            raise DiartAmdError(f"DZ_EXPERIMENTS=1 but {_LIB_PATH} is not an experiments build")
        sizes = (C.c_int * 5)()
        lib.dz_abi_struct_sizes(C.byref(sizes))
        mine = [C.sizeof(t) for t in (SincNetWeights, SegWeights, EmbWeights, EcapaWeights, ConvGemmDesc)]
        if list(sizes) != mine:
            raise DiartAmdError(f"{_LIB_PATH} was built from a different include/diart_amd.h: struct sizes "
                                f"{list(sizes)} (library) vs {mine} (this binding); rebuild it")
        for name, struct in (("dz_wsp", WspWeights), ("dz_sbx", SbxWeights), ("dz_ttn", TtnWeights),
                             ("dz_sbr", SbrWeights), ("dz_ecm", EcmWeights), ("dz_tune", TuneDesc),
                             ("dz_tune_cells", TuneCells)):
            size = getattr(lib, f"{name}_abi_size")()
            if size != C.sizeof(struct):
                what = {TuneDesc: "dz_tune_desc", TuneCells: "dz_tune_cells"}.get(struct, f"{name}_weights")
                raise DiartAmdError(f"{_LIB_PATH} was built from a different include/diart_amd.h: sizeof({what}) "
                                    f"{size} (library) vs {C.sizeof(struct)} (this binding); rebuild it")
        _lib = lib
    return _lib


def experiments() -> bool:
    """Is the loaded library the experiments build?  (The shipped one ignores every kernel-selection switch.)"""
    return bool(load().dz_has_experiments())


def exp_env(name: str, default: str) -> str:
    """A DZ_* switch that only the experiments build honours: `default` in the shipped configuration."""
    return os.environ.get(name, default) if EXPERIMENTS else default


def set_option(name: str, value: int) -> None:
    check(load().dz_set_option(name.encode(), int(value)), "dz_set_option")


def get_option(name: str) -> int:
    v = C.c_int()
    check(load().dz_get_option(name.encode(), C.byref(v)), "dz_get_option")
    return v.value


_hip: Optional[C.CDLL] = None


def memcpy(dst: int, src, nbytes: int) -> None:
    """``hipMemcpy`` of ``nbytes`` between two device addresses (a handle's buffer into a tensor: ``peek``); the caller
    has synchronised the device."""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
    rc = _hip.hipMemcpy(vp(dst), src, C.c_size_t(nbytes), 3)     # hipMemcpyDeviceToDevice
    if rc != 0:
        raise DiartAmdError(f"hipMemcpy failed ({rc})")


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().dz_last_error().decode("utf-8", "replace")
        raise DiartAmdError(f"{what or 'libdiart_amd'} failed (code {rc}): {msg}")


_contexts = {}


def range_check(device_index: int, reset: bool = True) -> None:
    """Raise if a split-f16 kernel of this GPU's context met an operand outside +-65504 (it was
    clamped) since the last check.  The caller has synchronised the stream(s) that did the work."""
    ctx = _contexts.get(device_index)
    if ctx is not None:
        check(load().dz_range_check(ctx, int(reset)), "f16x3 operand range")


def context(device_index: int) -> vp:
    """One dz_ctx per (process, GPU)."""
    if device_index not in _contexts:
        h = vp()
        check(load().dz_ctx_create(int(device_index), C.byref(h)), "dz_ctx_create")
        _contexts[device_index] = h
    return _contexts[device_index]
