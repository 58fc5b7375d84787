"""ctypes binding of the C ABI in include/ppgs_amd.h (libppgs_amd.so).

PyTorch-ROCm supplies device memory (tensors), the current HIP stream and the
device index; all arithmetic happens in the HIP library.  There is no CPU or
eager-PyTorch fallback: if the library is missing or no GPU is visible the
calls raise.
"""
import collections
import ctypes
import math
import os
import threading

import torch

from . import config, weights

PPG_MAX_LAYERS = 16
PRECISIONS = {'fp32': 0, 'bf16': 1, 'fp16': 2, 'fp16x2': 3}
KERNEL_CLASSES = (
    'gather', 'inconv', 'qkv', 'attention', 'outproj_ln', 'ffn',
    'outconv_softmax', 'frontend')

# PPGS_AMD_LIB: an alternative build of the same library (kernel experiments)
_LIB_PATH = os.environ.get('PPGS_AMD_LIB') or os.path.join(
    os.path.dirname(os.path.abspath(__file__)), 'libppgs_amd.so')
_lib = None
_lib_lock = threading.Lock()

_FP = ctypes.POINTER(ctypes.c_float)


class PpgConfig(ctypes.Structure):
    _fields_ = [(name, ctypes.c_int32) for name in (
        'input_channels', 'hidden_channels', 'num_layers', 'ffn_channels',
        'output_channels', 'kernel_size', 'heads', 'is_causal',
        'max_positions', 'chunk_length', 'chunk_overlap', 'precision')]


class PpgWeights(ctypes.Structure):
    _fields_ = (
        [('position_encoding', _FP), ('input_weight', _FP), ('input_bias', _FP)] +
        [(name, _FP * PPG_MAX_LAYERS) for name in (
            'in_proj_weight', 'in_proj_bias', 'out_proj_weight',
            'out_proj_bias', 'linear1_weight', 'linear1_bias',
            'linear2_weight', 'linear2_bias', 'norm1_weight', 'norm1_bias',
            'norm2_weight', 'norm2_bias')] +
        [('output_weight', _FP), ('output_bias', _FP)])


class PpgWindow(ctypes.Structure):
    _fields_ = [(name, ctypes.c_int32) for name in (
        'item', 'chunked', 'start', 'frames', 'valid', 'keep_lo', 'keep_hi',
        'out_frame', 'tok_off', 'vt_off', 'pad0', 'pad1')]


class PpgW2v2LayerWeights(ctypes.Structure):
    _fields_ = [(name, ctypes.POINTER(ctypes.c_float)) for name in (
        'q_weight', 'q_bias', 'k_weight', 'k_bias', 'v_weight', 'v_bias', 'out_weight', 'out_bias',
        'norm1_weight', 'norm1_bias', 'ffn1_weight', 'ffn1_bias', 'ffn2_weight', 'ffn2_bias',
        'norm2_weight', 'norm2_bias')]


class PpgW2v2BodyWeights(ctypes.Structure):
    _fields_ = [
        ('hidden', ctypes.c_int32), ('heads', ctypes.c_int32), ('ffn', ctypes.c_int32),
        ('num_layers', ctypes.c_int32), ('conv_kernel', ctypes.c_int32), ('conv_groups', ctypes.c_int32),
        ('layer_norm_eps', ctypes.c_float), ('pad0', ctypes.c_int32)] + [
        (name, ctypes.POINTER(ctypes.c_float)) for name in (
            'proj_norm_weight', 'proj_norm_bias', 'proj_weight', 'proj_bias',
            'pos_conv_weight', 'pos_conv_bias', 'enc_norm_weight', 'enc_norm_bias')] + [
        ('layers', PpgW2v2LayerWeights * 24)]


class PpgAttentionItem(ctypes.Structure):
    _fields_ = [(name, ctypes.c_int32) for name in (
        'window', 'q0', 'queries', 'frames', 'valid', 'narrow')]


class PpgPlanInfo(ctypes.Structure):
    _fields_ = [
        ('num_windows', ctypes.c_int32), ('skipped_windows', ctypes.c_int32),
        ('tokens', ctypes.c_int32), ('vt_tokens', ctypes.c_int32),
        ('processed_frames', ctypes.c_int64),
        ('attention_pairs', ctypes.c_int64),
        ('workspace_bytes', ctypes.c_size_t)]


class PpgMetricsState(ctypes.Structure):
    """The device block of ppg_metrics_update: 64-bit integers, real-valued sums in units of 2^-32."""
    _fields_ = [(name, ctypes.c_int64) for name in (
        'count', 'true_positives', 'topk_correct', 'invalid_labels', 'loss_sum', 'loss_weight_sum',
        'jsd_sum', 'reserved')] + [
        ('class_total', ctypes.c_int64 * 40), ('class_count', ctypes.c_int64 * 40),
        ('distance_matrix', ctypes.c_int64 * 40 * 40), ('confusion', ctypes.c_int64 * 40 * 40)]


# every symbol include/ppgs_amd.h declares: name -> (restype, argtypes)
_I64P = ctypes.POINTER(ctypes.c_int64)
SYMBOLS = {
    'ppg_last_error': (ctypes.c_char_p, []),
    'ppg_abi_version': (ctypes.c_int, []),
    'ppg_engine_create': (ctypes.c_int, [
        ctypes.POINTER(PpgConfig), ctypes.POINTER(PpgWeights), ctypes.c_int,
        ctypes.POINTER(ctypes.c_void_p)]),
    'ppg_engine_destroy': (None, [ctypes.c_void_p]),
    'ppg_plan_windows': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _I64P, ctypes.c_int,
        ctypes.POINTER(PpgWindow), ctypes.c_int, ctypes.POINTER(PpgPlanInfo)]),
    'ppg_plan_attention_items': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _I64P, ctypes.c_int, ctypes.c_int,
        ctypes.POINTER(PpgAttentionItem), ctypes.c_int]),
    'ppg_workspace_bytes': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _I64P, ctypes.c_int,
        ctypes.POINTER(ctypes.c_size_t)]),
    'ppg_encode': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, _I64P, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'ppg_frontend': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_audio_stream_frames': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int]),
    'ppg_frontend_stream_create': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    'ppg_frontend_stream_destroy': (None, [ctypes.c_void_p]),
    'ppg_frontend_stream_batch': (ctypes.c_int, [ctypes.c_void_p]),
    'ppg_frontend_stream_state': (ctypes.c_int, [ctypes.c_void_p, _I64P, _I64P]),
    'ppg_frontend_stream_reset': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'ppg_frontend_stream_push': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
        ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, _I64P,
        ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]),
    'ppg_resample_length': (ctypes.c_int64, [
        ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    'ppg_resample': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
        ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_distance': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_sparsify': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_grid_sample': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_dtw_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'ppg_dtw': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'ppg_edit_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'ppg_edit_distance': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'ppg_align_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'ppg_align': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_size_t, ctypes.c_void_p]),
    'ppg_align_optional_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'ppg_align_optional': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'ppg_decode': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_recognize_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    'ppg_recognize': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'ppg_viterbi_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'ppg_viterbi': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'ppg_posterior_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'ppg_posterior': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'ppg_search_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'ppg_search': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_size_t, ctypes.c_void_p]),
    'ppg_search_graph_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'ppg_search_graph': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_float,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'ppg_search_stream_state_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'ppg_search_stream_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'ppg_search_stream_reset': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_search_stream_push': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'ppg_search_stream_flush': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_search_graph_stream_state_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'ppg_search_graph_stream_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'ppg_search_graph_stream_open': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_search_graph_stream_reset': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_search_graph_stream_push': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_int,
        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'ppg_search_graph_stream_flush': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_recognize_stream_state_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    'ppg_recognize_stream_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    'ppg_recognize_stream_reset': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_recognize_stream_push': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
        ctypes.c_void_p]),
    'ppg_recognize_stream_flush': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_viterbi_stream_state_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'ppg_viterbi_stream_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    'ppg_viterbi_stream_open': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_viterbi_stream_reset': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_viterbi_stream_push': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'ppg_viterbi_stream_flush': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_posterior_stream_emitted': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    'ppg_posterior_stream_block': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                                    ctypes.c_int64]),
    'ppg_posterior_stream_state_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'ppg_posterior_stream_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    'ppg_posterior_stream_open': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'ppg_posterior_stream_reset': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_posterior_stream_push': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'ppg_posterior_stream_flush': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_metrics_state_bytes': (ctypes.c_size_t, []),
    'ppg_metrics_reset': (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_metrics_update': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'ppg_w2v2_body_create': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    'ppg_w2v2_body_destroy': (None, [ctypes.c_void_p]),
    'ppg_w2v2_body_workspace_bytes': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    'ppg_w2v2_body_forward': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, _I64P, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'ppg_stream_create': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    'ppg_stream_destroy': (None, [ctypes.c_void_p]),
    'ppg_stream_rows': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
        ctypes.POINTER(ctypes.c_int)]),
    'ppg_stream_posteriors': (ctypes.c_void_p, [ctypes.c_void_p]),
    'ppg_stream_push': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]),
    'ppg_engine_nonfinite': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    'ppg_engine_pipelines': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'ppg_stream_create_batch': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    'ppg_stream_batch': (ctypes.c_int, [ctypes.c_void_p]),
    'ppg_stream_push_batch': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
        ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]),
    'ppg_w2v2_create': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    'ppg_w2v2_destroy': (None, [ctypes.c_void_p]),
    'ppg_w2v2_frames': (ctypes.c_int64, [ctypes.c_int64]),
    'ppg_w2v2_workspace_bytes': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_size_t)]),
    'ppg_w2v2_features': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'ppg_engine_profile': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'ppg_engine_profile_read': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
        _I64P]),
    'ppg_engine_profile_reset': (ctypes.c_int, [ctypes.c_void_p]),
    'ppg_engine_profile_stride': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'ppg_frontend_profile': (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    'ppg_frontend_profile_read': (ctypes.c_int, [
        ctypes.c_int, ctypes.POINTER(ctypes.c_double), _I64P]),
    'ppg_io_last_error': (ctypes.c_char_p, []),
    'ppg_wav_info': (ctypes.c_int, [
        ctypes.c_char_p, _I64P, ctypes.POINTER(ctypes.c_int32),
        ctypes.POINTER(ctypes.c_int32)]),
    'ppg_wav_read_batch': (ctypes.c_int, [
        ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.c_void_p,
        ctypes.c_int64, ctypes.c_int64, _I64P,
        ctypes.POINTER(ctypes.c_int32), ctypes.c_int]),
    'ppg_pt_write_batch': (ctypes.c_int, [
        ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.c_void_p,
        ctypes.c_int64, ctypes.c_int, ctypes.c_int64, _I64P, ctypes.c_int]),
}


def library_sha16(path=None):
    """First 16 hex digits of the sha256 of the built library (a clean `make` reproduces it byte for byte): what binds a
    committed rocprofv3 counter summary (profiles/r*_pmc_summary*.txt, header `# lib_sha256_16=`) to a build."""
    import hashlib
    with open(path or _LIB_PATH, 'rb') as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def library():
    """Load libppgs_amd.so (built in-tree by __graft_entry__.build / make)."""
    global _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(_LIB_PATH):
                raise RuntimeError(
                    f'{_LIB_PATH} is missing: build it with '
                    '`python -c "import __graft_entry__ as g; g.build()"` or '
                    '`make -C ppgs_amd/csrc`. The PPG engine has no fallback '
                    'path.')
            lib = ctypes.CDLL(_LIB_PATH)
            for name, (restype, argtypes) in SYMBOLS.items():
                fn = getattr(lib, name)
                fn.restype = restype
                fn.argtypes = argtypes
            _lib = lib
    return _lib


class PpgError(RuntimeError):
    pass


_ERRORS = {-1: ValueError, -2: PpgError, -3: PpgError, -4: ValueError}


def _check(code):
    if code < 0:
        message = library().ppg_last_error().decode()
        raise _ERRORS.get(code, PpgError)(f'ppgs_amd: {message} (code {code})')
    return code


def _lengths_array(lengths, batch):
    if isinstance(lengths, torch.Tensor):
        lengths = lengths.detach().cpu().reshape(-1).tolist()
    elif isinstance(lengths, int):
        lengths = [lengths]
    lengths = [int(v) for v in lengths]
    if len(lengths) != batch:
        raise ValueError(
            f'lengths has {len(lengths)} entries for a batch of {batch}')
    return (ctypes.c_int64 * batch)(*lengths)


def plan_windows(batch, frames, lengths, legacy_mode=False, engine=None):
    """Host-only chunk plan (works without a GPU): (windows, info)."""
    lib = library()
    arr = _lengths_array(lengths, batch)
    info = PpgPlanInfo()
    handle = engine._handle if engine is not None else None
    count = _check(lib.ppg_plan_windows(
        handle, batch, frames, arr, int(legacy_mode), None, 0,
        ctypes.byref(info)))
    windows = (PpgWindow * max(count, 1))()
    _check(lib.ppg_plan_windows(
        handle, batch, frames, arr, int(legacy_mode), windows, count,
        ctypes.byref(info)))
    return list(windows)[:count], info


def plan_attention_items(batch, frames, lengths, legacy_mode=False, heads=config.ATTENTION_HEADS, engine=None):
    """Host-only: the attention work items of a batch in launch order (ppg_plan_attention_items)."""
    lib = library()
    arr = _lengths_array(lengths, batch)
    handle = engine._handle if engine is not None else None
    count = _check(lib.ppg_plan_attention_items(handle, batch, frames, arr, int(legacy_mode), heads, None, 0))
    items = (PpgAttentionItem * max(count, 1))()
    _check(lib.ppg_plan_attention_items(handle, batch, frames, arr, int(legacy_mode), heads, items, count))
    return list(items)[:count]


class Engine:
    """One loaded PPG network on one GPU (mirrors the per-model cache of
    reference ppgs.infer, ppgs/core.py:565-583)."""

    def __init__(self, state, device=0, precision='bf16', is_causal=False,
                 heads=config.ATTENTION_HEADS):
        if not torch.cuda.is_available():
            raise PpgError(
                'ppgs_amd: no HIP device visible; the engine has no CPU path')
        lib = library()
        cin, hidden, layers = weights.geometry(state)
        if layers > PPG_MAX_LAYERS:     # (PpgWeights has that many slots per parameter: refused before they are filled)
            raise ValueError(f'ppgs_amd: num_layers {layers} outside [0,{PPG_MAX_LAYERS}]')
        self.input_channels = cin
        self.hidden_channels = hidden
        self.output_channels = state['output_layer.weight'].shape[0]
        self.precision = precision
        self.is_causal = bool(is_causal)
        self.device = torch.device('cuda', device)
        cfg = PpgConfig(
            input_channels=cin, hidden_channels=hidden, num_layers=layers,
            ffn_channels=(
                state['model.layers.0.linear1.weight'].shape[0]
                if layers else config.FFN_CHANNELS),
            output_channels=self.output_channels,
            kernel_size=state['input_layer.weight'].shape[2], heads=heads,
            is_causal=int(is_causal),
            max_positions=state['position.encoding'].shape[0],
            chunk_length=config.CHUNK_LENGTH,
            chunk_overlap=config.CHUNK_OVERLAP,
            precision=PRECISIONS[precision])
        keep = []

        def ptr(key):
            tensor = state[key].detach().to('cpu', torch.float32).contiguous()
            keep.append(tensor)
            return ctypes.cast(tensor.data_ptr(), _FP)
        wts = PpgWeights()
        wts.position_encoding = ptr('position.encoding')
        wts.input_weight = ptr('input_layer.weight')
        wts.input_bias = ptr('input_layer.bias')
        wts.output_weight = ptr('output_layer.weight')
        wts.output_bias = ptr('output_layer.bias')
        names = {
            'in_proj_weight': 'self_attn.in_proj_weight',
            'in_proj_bias': 'self_attn.in_proj_bias',
            'out_proj_weight': 'self_attn.out_proj.weight',
            'out_proj_bias': 'self_attn.out_proj.bias',
            'linear1_weight': 'linear1.weight', 'linear1_bias': 'linear1.bias',
            'linear2_weight': 'linear2.weight', 'linear2_bias': 'linear2.bias',
            'norm1_weight': 'norm1.weight', 'norm1_bias': 'norm1.bias',
            'norm2_weight': 'norm2.weight', 'norm2_bias': 'norm2.bias'}
        for field, key in names.items():
            array = getattr(wts, field)
            for l in range(layers):
                array[l] = ptr(f'model.layers.{l}.{key}')
        handle = ctypes.c_void_p()
        _check(lib.ppg_engine_create(
            ctypes.byref(cfg), ctypes.byref(wts), device, ctypes.byref(handle)))
        self._handle = handle
        self._lib = lib
        self._workspaces = {}         # one scratch buffer per HIP stream in use

    def __del__(self):
        handle = getattr(self, '_handle', None)
        if handle:
            self._lib.ppg_engine_destroy(handle)
            self._handle = None

    def workspace_bytes(self, batch, frames, lengths, legacy_mode=False):
        size = ctypes.c_size_t()
        _check(self._lib.ppg_workspace_bytes(
            self._handle, batch, frames, _lengths_array(lengths, batch),
            int(legacy_mode), ctypes.byref(size)))
        return size.value

    def stream(self, max_frames, dtype=torch.float16):
        """A KV-cached causal stream over one utterance of up to `max_frames` frames
        (see Stream); the engine must be causal."""
        return Stream(self, max_frames, dtype)

    def pipelines(self, tokens):
        """HIP streams a batch of `tokens` token rows (PlanInfo.tokens) is split over (1 or 2)."""
        return int(self._lib.ppg_engine_pipelines(self._handle, int(tokens)))

    def nonfinite(self, clear=True):
        """True when a launch of this engine produced a non-finite logit for a valid frame since the
        flag was last cleared (synchronises with the device): fp16 operands past 65504, or
        non-finite input features."""
        flag = ctypes.c_int()
        with torch.cuda.device(self.device):
            _check(self._lib.ppg_engine_nonfinite(self._handle, int(clear), ctypes.byref(flag)))
        return bool(flag.value)

    def check_finite(self):
        """Raise PpgError if nonfinite() (and clear the flag)."""
        if self.nonfinite(clear=True):
            raise PpgError(
                f'ppgs_amd: non-finite logits ({self.precision} operands): an activation left the operand '
                "format's range (fp16: |x| < 65504) or the input features are not finite; "
                'PPGS_AMD_PRECISION=bf16 or fp32 has the range of fp32')

    def batched_stream(self, batch, max_frames, dtype=torch.float16):
        """KV-cached causal streams over `batch` utterances advanced together (see
        BatchedStream); the engine must be causal."""
        return BatchedStream(self, batch, max_frames, dtype)

    def long_stream(self, dtype=torch.float16):
        """A KV-cached causal stream over an utterance of any length > 500 frames
        (see LongStream); the engine must be causal."""
        return LongStream(self, dtype)

    def audio_stream(self, max_frames, max_push_samples=16000):
        """Stream.push for raw 16 kHz samples (see AudioStream): causal engines with 80 input channels."""
        return AudioStream(self, max_frames, max_push_samples)

    def batched_audio_stream(self, batch, max_frames, max_push_samples=16000):
        """BatchedStream.push for raw 16 kHz samples (see BatchedAudioStream)."""
        return BatchedAudioStream(self, batch, max_frames, max_push_samples)

    def long_audio_stream(self, max_push_samples=16000):
        """LongStream.push for raw 16 kHz samples (see LongAudioStream)."""
        return LongAudioStream(self, max_push_samples)

    def encode(self, features, lengths, softmax=True, legacy_mode=False,
               workspace=None):
        """features (B, Cin, T) fp16/fp32 on this engine's GPU -> (B, 40, T)
        fp32 on the same GPU (posteriors, or logits if softmax=False).
        `workspace`: a caller-owned uint8 scratch tensor of at least
        workspace_bytes(); default: one grow-only buffer per HIP stream."""
        if features.dim() != 3 or features.shape[1] != self.input_channels:
            raise ValueError(
                f'features must be (batch, {self.input_channels}, frames), '
                f'got {tuple(features.shape)}')
        features = features.to(self.device)
        if features.dtype == torch.float16:
            dtype = 0
        else:
            features = features.to(torch.float32)
            dtype = 1
        features = features.contiguous()
        batch, _, frames = features.shape
        arr = _lengths_array(lengths, batch)
        size = ctypes.c_size_t()
        _check(self._lib.ppg_workspace_bytes(
            self._handle, batch, frames, arr, int(legacy_mode),
            ctypes.byref(size)))
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
            # encodes issued on different streams may overlap: each stream
            # gets its own scratch buffer (grow-only, reused call to call)
            if workspace is not None:
                if workspace.numel() < size.value or workspace.device != self.device:
                    raise ValueError(
                        f'workspace of {workspace.numel()} bytes, {size.value} needed')
            else:
                workspace = self._workspaces.get(stream)
                if workspace is None or workspace.numel() < size.value:
                    # (zeros: nothing reads a byte it has not written -- test_poisoned_workspace -- but a grow-only
                    # buffer allocated once may as well start defined)
                    workspace = torch.zeros(
                        max(size.value, 256), dtype=torch.uint8, device=self.device)
                    # a buffer allocated under stream capture lives in the graph's
                    # private pool: never cache it for later eager calls
                    if not torch.cuda.is_current_stream_capturing():
                        self._workspaces[stream] = workspace
            out = torch.empty(
                (batch, self.output_channels, frames), dtype=torch.float32,
                device=self.device)
            _check(self._lib.ppg_encode(
                self._handle, features.data_ptr(), dtype, arr, batch, frames,
                int(softmax), int(legacy_mode), out.data_ptr(),
                workspace.data_ptr(), workspace.numel(), stream))
        return out

    # -- HIP-graph replay for launch-bound shapes ---------------------------
    def graphed(self, batch, frames, lengths=None, softmax=True,
                legacy_mode=False, feature_dtype=torch.float16):
        """A replayable encode for one fixed (batch, frames, lengths) shape:
        the ~30 launches of ppg_encode captured once into a HIP graph (the
        plan is cached and nothing inside allocates or synchronises), e.g.
        the streaming configuration -- 64 causal 160-frame chunks per step --
        where launch latency, not kernel time, sets the step rate.

        Returns ``run(features) -> posteriors``; the returned tensor is a
        static buffer overwritten by the next call.  ``run.static_input`` is
        the buffer the graph reads: a producer that writes it in place calls
        ``run()`` without an argument and saves the copy.
        """
        lengths = [frames] * batch if lengths is None else lengths
        static_in = torch.zeros(
            (batch, self.input_channels, frames), dtype=feature_dtype,
            device=self.device)
        # the graph gets a scratch buffer of its own (two graphs of one engine replayed on
        # different streams must not share one), allocated before the capture starts
        scratch = torch.empty(
            max(self.workspace_bytes(batch, frames, lengths, legacy_mode), 256),
            dtype=torch.uint8, device=self.device)
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(2):                       # the window plan is built, uploaded and cached here
                self.encode(static_in, lengths, softmax, legacy_mode, workspace=scratch)
        torch.cuda.current_stream(self.device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            # (under capture ppg_encode pins the cached plan: the graph holds its device pointers)
            static_out = self.encode(static_in, lengths, softmax, legacy_mode, workspace=scratch)

        def run(features=None):
            # features=None: the caller's producer (e.g. the mel frontend) wrote run.static_input in place
            if features is not None:
                static_in.copy_(features, non_blocking=True)
            graph.replay()
            return static_out
        run.graph = graph
        run.scratch = scratch
        run.static_input = static_in
        run.static_output = static_out
        return run

    # -- per-kernel HIP-event timing (bench.py roofline leg) ----------------
    def profile(self, enable=True, classes=None, stride=1):
        """Time launches with HIP events: every kernel class, or only the
        named ones (each timed launch adds two event records to the stream);
        stride n times every n-th launch of a class only."""
        _check(self._lib.ppg_engine_profile_stride(self._handle, int(stride)))
        mask = 0
        if enable:
            mask = -1 if classes is None else sum(
                1 << KERNEL_CLASSES.index(name) for name in classes)
        _check(self._lib.ppg_engine_profile(self._handle, mask))
        _check(self._lib.ppg_engine_profile_reset(self._handle))

    def profile_read(self):
        """{kernel class: (total ms, launches)} since profile(True)."""
        result = {}
        for index, name in enumerate(KERNEL_CLASSES[:-1]):
            total, count = ctypes.c_double(), ctypes.c_int64()
            _check(self._lib.ppg_engine_profile_read(
                self._handle, index, ctypes.byref(total), ctypes.byref(count)))
            result[name] = (total.value, count.value)
        return result


def frontend(audio, spectrogram=False, mel=True):
    """audio (B, 1, N) or (B, N) fp32 on a GPU -> fp16 spectrogram (B,513,T)
    and/or log-mel (B,80,T) on the same GPU, T = N // 160."""
    if not audio.is_cuda:
        raise PpgError('ppgs_amd: frontend input must live on a HIP device')
    if audio.dim() == 3:
        if audio.shape[1] != 1:
            raise ValueError(f'audio must be (batch, 1, samples), got {tuple(audio.shape)}')
        audio = audio[:, 0]
    audio = audio.to(torch.float32).contiguous()
    batch, samples = audio.shape
    frames = samples // config.HOPSIZE
    spec_out = mel_out = None
    if spectrogram:
        spec_out = torch.empty(
            (batch, config.NUM_BINS, frames), dtype=torch.float16,
            device=audio.device)
    if mel:
        mel_out = torch.empty(
            (batch, config.NUM_MELS, frames), dtype=torch.float16,
            device=audio.device)
    lib = library()
    with torch.cuda.device(audio.device):
        stream = torch.cuda.current_stream().cuda_stream
        _check(lib.ppg_frontend(
            audio.device.index, audio.data_ptr(), batch, samples,
            spec_out.data_ptr() if spectrogram else None,
            mel_out.data_ptr() if mel else None, stream))
    return spec_out, mel_out


def resample(audio, sample_rate, target_rate=config.SAMPLE_RATE):
    """(..., samples) fp32 on a GPU at sample_rate -> (..., samples') at
    target_rate, torchaudio.transforms.Resample defaults (ppg_resample)."""
    if not audio.is_cuda:
        raise PpgError('ppgs_amd: the native resampler works on a HIP device tensor')
    shape = audio.shape
    flat = audio.reshape(-1, shape[-1]).to(torch.float32).contiguous()
    lib = library()
    length = lib.ppg_resample_length(flat.shape[1], int(sample_rate), int(target_rate))
    out = torch.empty((flat.shape[0], length), dtype=torch.float32, device=audio.device)
    with torch.cuda.device(audio.device):
        _check(lib.ppg_resample(
            audio.device.index, flat.data_ptr(), flat.shape[0], flat.shape[1],
            int(sample_rate), int(target_rate), out.data_ptr(),
            torch.cuda.current_stream().cuda_stream))
    return out.reshape(shape[:-1] + (length,))


def distance_frames(ppg_x, ppg_y, mix=None):
    """Per-frame similarity-weighted Jensen-Shannon term (ppg_distance):
    (40, frames) x 2 on a GPU [+ (40, 40) mixing matrix] -> (frames,)."""
    if not (ppg_x.is_cuda and ppg_y.is_cuda):
        raise PpgError('ppgs_amd: the post-ops work on HIP device tensors')
    x = ppg_x.to(torch.float32).contiguous()
    y = ppg_y.to(torch.float32).contiguous()
    if x.shape != y.shape or x.dim() != 2 or x.shape[0] != 40:
        raise ValueError(f'PPGs must both be (40, frames), got {tuple(x.shape)} and {tuple(y.shape)}')
    if mix is not None:
        mix = mix.to(device=x.device, dtype=torch.float32).contiguous()
    out = torch.empty((x.shape[1],), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(library().ppg_distance(
            x.device.index, x.data_ptr(), y.data_ptr(), x.shape[1],
            mix.data_ptr() if mix is not None else None, out.data_ptr(),
            torch.cuda.current_stream().cuda_stream))
    return out


def sparsify(ppg, method, threshold):
    """(batch, 40, frames) on a GPU -> same shape (ppg_sparsify); method 0
    constant / 1 percentile / 2 topk, one threshold."""
    if not ppg.is_cuda:
        raise PpgError('ppgs_amd: the post-ops work on HIP device tensors')
    x = ppg.to(torch.float32).contiguous()
    if x.dim() != 3 or x.shape[1] != 40:
        raise ValueError(f'PPG must be (batch, 40, frames), got {tuple(x.shape)}')
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _check(library().ppg_sparsify(
            x.device.index, x.data_ptr(), x.shape[0], x.shape[2], int(method),
            float(threshold), out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return out


def grid_sample(ppg, grid):
    """(..., frames) on a GPU sampled at the fractional frame indices `grid`
    (length,) -> (..., length) (ppg_grid_sample)."""
    if not ppg.is_cuda:
        raise PpgError('ppgs_amd: the post-ops work on HIP device tensors')
    if grid.dim() != 1:
        raise ValueError(f'grid must be one-dimensional, got {tuple(grid.shape)}')
    if ppg.dim() < 1 or ppg.shape[-1] < 1:
        raise ValueError(f'PPG must be (..., frames >= 1), got {tuple(ppg.shape)}')
    x = ppg.to(torch.float32).contiguous()
    g = grid.to(device=x.device, dtype=torch.float32).contiguous()
    out = torch.empty(x.shape[:-1] + (g.shape[0],), dtype=torch.float32, device=x.device)
    rows = x.numel() // x.shape[-1]
    if rows and g.shape[0]:
        with torch.cuda.device(x.device):
            _check(library().ppg_grid_sample(
                x.device.index, x.data_ptr(), rows, x.shape[-1], g.data_ptr(),
                g.shape[0], out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return out      # fp32 also for half-precision PPGs: the reference's float grid promotes them


DTW_MAX_FRAMES = 4096          # PPG_DTW_MAX_FRAMES
DTW_MAX_PAIRS = 65535          # PPG_DTW_MAX_PAIRS, per call of the library
DTW_WORKSPACE_BYTES = 4 << 30  # a larger batch runs as several calls, each within this much workspace


def dtw_pairs(ppg_x, ppg_y, lengths_x, lengths_y, mix=None, want_path=False, want_cost=False):
    """Dynamic time warping of pair b = (ppg_x[b, :, :lengths_x[b]], ppg_y[b, :, :lengths_y[b]]) over the
    per-frame term of ppg_distance (ppg_dtw): (pairs, 40, frames_x) and (pairs, 40, frames_y) on a GPU, lengths as
    host integers -> total (pairs,) fp32, steps (pairs,) int32, and with want_path the padded paths
    (pairs, frames_x + frames_y - 1, 2) int32 [and with want_cost the cell costs along them], else None."""
    if not (ppg_x.is_cuda and ppg_y.is_cuda):
        raise PpgError('ppgs_amd: the post-ops work on HIP device tensors')
    x = ppg_x.to(torch.float32).contiguous()
    y = ppg_y.to(torch.float32).contiguous()
    if x.dim() != 3 or y.dim() != 3 or x.shape[1] != 40 or y.shape[1] != 40 or x.shape[0] != y.shape[0]:
        raise ValueError(f'PPGs must be (pairs, 40, frames), got {tuple(x.shape)} and {tuple(y.shape)}')
    pairs, frames_x, frames_y = x.shape[0], x.shape[2], y.shape[2]
    if not (1 <= frames_x <= DTW_MAX_FRAMES and 1 <= frames_y <= DTW_MAX_FRAMES and pairs >= 1):
        raise ValueError(f'dtw takes 1 to {DTW_MAX_FRAMES} frames per side, got {frames_x} and {frames_y}')
    want_path = want_path or want_cost
    device = x.device
    if mix is not None:
        mix = mix.to(device=device, dtype=torch.float32).contiguous()
    lengths = torch.tensor([list(lengths_x), list(lengths_y)], dtype=torch.int32).to(device)
    total = torch.empty((pairs,), dtype=torch.float32, device=device)
    steps = torch.empty((pairs,), dtype=torch.int32, device=device)
    longest = frames_x + frames_y - 1
    path = torch.zeros((pairs, longest, 2), dtype=torch.int32, device=device) if want_path else None
    path_length = torch.empty((pairs,), dtype=torch.int32, device=device) if want_path else None     # K again
    cost = torch.zeros((pairs, longest), dtype=torch.float32, device=device) if want_cost else None
    lib = library()
    per_pair = lib.ppg_dtw_workspace_bytes(1, frames_x, frames_y, int(want_path))
    group = max(1, min(pairs, DTW_MAX_PAIRS, DTW_WORKSPACE_BYTES // per_pair))
    size = lib.ppg_dtw_workspace_bytes(group, frames_x, frames_y, int(want_path))
    workspace = torch.empty((size,), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        for at in range(0, pairs, group):
            count = min(group, pairs - at)
            _check(lib.ppg_dtw(
                device.index, x[at:].data_ptr(), frames_x, y[at:].data_ptr(), frames_y, count,
                lengths[0, at:].data_ptr(), lengths[1, at:].data_ptr(),
                mix.data_ptr() if mix is not None else None, total[at:].data_ptr(), steps[at:].data_ptr(),
                path[at:].data_ptr() if want_path else None,
                path_length[at:].data_ptr() if want_path else None,
                cost[at:].data_ptr() if want_cost else None,
                workspace.data_ptr(), size, stream))
    return total, steps, path, cost


EDIT_MAX_TOKENS = 4096          # PPG_EDIT_MAX_TOKENS
EDIT_MAX_PAIRS = 65535          # PPG_EDIT_MAX_PAIRS, per call of the library
EDIT_STATISTICS = 41 * 41 + 2   # PPG_EDIT_STATISTICS: the (41, 41) table, then the valid and the invalid pairs
EDIT_WORKSPACE_BYTES = 1 << 30  # a larger batch runs as several calls, each within this much workspace


def edit_pairs(ref, hyp, lengths_ref, lengths_hyp, costs=None, want_ops=False, statistics=None):
    """Weighted edit distance of pair b = (ref[b, :lengths_ref[b]], hyp[b, :lengths_hyp[b]]) (ppg_edit_distance):
    padded int32 (pairs, tokens_ref) and (pairs, tokens_hyp) on a GPU; lengths as host integers or as int32 device
    tensors; `costs` None for the unit costs or device fp32 (sub (40, 40), del (40,), ins (40,)) -> total (pairs,) fp32,
    counts (pairs, 4) int32 = hits, substitutions, deletions, insertions, and with want_ops the padded operations
    (pairs, tokens_ref + tokens_hyp, 3) int32 and their number K (pairs,) int32, else None.  `statistics`, an int64
    device tensor of EDIT_STATISTICS words, is added to; without want_ops the operations it is made from live in a
    buffer of one group of pairs and only K is returned.  With want_ops the padded operations of the WHOLE batch are
    an output, 12 (tokens_ref + tokens_hyp) bytes per pair outside the workspace cap.  Nothing here waits for the
    device."""
    if not (torch.is_tensor(ref) and torch.is_tensor(hyp) and ref.is_cuda and hyp.is_cuda):
        raise PpgError('ppgs_amd: the post-ops work on HIP device tensors')
    if ref.dim() != 2 or hyp.dim() != 2 or ref.shape[0] != hyp.shape[0] or ref.shape[0] < 1 or \
            ref.dtype != torch.int32 or hyp.dtype != torch.int32:
        raise ValueError(f'token tables must be int32 (pairs >= 1, tokens), got {tuple(ref.shape)} {ref.dtype} and '
                         f'{tuple(hyp.shape)} {hyp.dtype}')
    pairs, tokens_ref, tokens_hyp = ref.shape[0], ref.shape[1], hyp.shape[1]
    if tokens_ref > EDIT_MAX_TOKENS or tokens_hyp > EDIT_MAX_TOKENS:
        raise ValueError(f'edit distance takes at most {EDIT_MAX_TOKENS} tokens per side, got {tokens_ref} and '
                         f'{tokens_hyp}')
    device = ref.device
    keep_ops = bool(want_ops)
    want_ops = keep_ops or statistics is not None
    if statistics is not None and not (
            torch.is_tensor(statistics) and statistics.device == device and statistics.dtype == torch.int64 and
            statistics.is_contiguous() and statistics.numel() == EDIT_STATISTICS):
        raise ValueError(f'statistics must be a contiguous int64 tensor of {EDIT_STATISTICS} words on {device}')
    if costs is not None:
        shapes = ((40, 40), (40,), (40,))
        if len(costs) != 3 or any(
                not torch.is_tensor(c) or c.device != device or c.dtype != torch.float32 or tuple(c.shape) != shape
                for c, shape in zip(costs, shapes)):
            raise ValueError(f'costs must be fp32 (40, 40), (40,), (40,) on {device}')
        costs = [c.contiguous() for c in costs]
    ref, hyp = ref.contiguous(), hyp.contiguous()
    lengths = []
    for value in (lengths_ref, lengths_hyp):
        if torch.is_tensor(value) and value.is_cuda:
            value = value.to(device=device, dtype=torch.int32).contiguous()
        else:
            value = torch.tensor([int(v) for v in value], dtype=torch.int32).to(device)
        if value.shape != (pairs,):
            raise ValueError(f'{value.numel()} lengths for {pairs} pairs')
        lengths.append(value)
    total = torch.empty((pairs,), dtype=torch.float32, device=device)
    counts = torch.empty((pairs, 4), dtype=torch.int32, device=device)
    ops_length = torch.empty((pairs,), dtype=torch.int32, device=device) if want_ops else None
    lib = library()
    per_pair = lib.ppg_edit_workspace_bytes(1, tokens_ref, tokens_hyp, int(want_ops))
    group = max(1, min(pairs, EDIT_MAX_PAIRS, EDIT_WORKSPACE_BYTES // per_pair))
    ops = None
    if keep_ops:
        ops = torch.zeros((pairs, tokens_ref + tokens_hyp, 3), dtype=torch.int32, device=device)
    elif want_ops:      # for the statistics only: one group's worth, written over by every call on this stream
        ops = torch.empty((group, tokens_ref + tokens_hyp, 3), dtype=torch.int32, device=device)
    size = lib.ppg_edit_workspace_bytes(group, tokens_ref, tokens_hyp, int(want_ops))
    workspace = torch.empty((size,), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        for at in range(0, pairs, group):
            count = min(group, pairs - at)
            _check(lib.ppg_edit_distance(
                device.index, ref[at:].data_ptr() if tokens_ref else None, tokens_ref,
                hyp[at:].data_ptr() if tokens_hyp else None, tokens_hyp, count,
                lengths[0][at:].data_ptr(), lengths[1][at:].data_ptr(),
                costs[0].data_ptr() if costs else None, costs[1].data_ptr() if costs else None,
                costs[2].data_ptr() if costs else None, total[at:].data_ptr(), counts[at:].data_ptr(),
                (ops[at:] if keep_ops else ops).data_ptr() if want_ops else None,
                ops_length[at:].data_ptr() if want_ops else None,
                statistics.data_ptr() if statistics is not None else None, workspace.data_ptr(), size, stream))
    return total, counts, ops if keep_ops else None, ops_length


ALIGN_MAX_FRAMES = 4096          # PPG_ALIGN_MAX_FRAMES
ALIGN_MAX_PHONEMES = 1024        # PPG_ALIGN_MAX_PHONEMES
ALIGN_MAX_ITEMS = 65535          # PPG_ALIGN_MAX_ITEMS, per call of the library
ALIGN_WORKSPACE_BYTES = 1 << 30  # a larger batch runs as several calls, each within this much workspace


def _items(ppg, lengths, what, most=ALIGN_MAX_FRAMES):
    """The checks and conversions align_items, decode_items and recognize_items share: (x, lengths as host integers)."""
    if not ppg.is_cuda:
        raise PpgError('ppgs_amd: the post-ops work on HIP device tensors')
    x = ppg.to(torch.float32).contiguous()
    if x.dim() != 3 or x.shape[1] != 40 or x.shape[0] < 1:
        raise ValueError(f'PPGs must be (items >= 1, 40, frames), got {tuple(x.shape)}')
    if not 1 <= x.shape[2] <= most:
        raise ValueError(f'{what} takes 1 to {most} frames, got {x.shape[2]}')
    lengths = [int(v) for v in lengths]
    if len(lengths) != x.shape[0]:
        raise ValueError(f'{len(lengths)} lengths for {x.shape[0]} items')
    return x, lengths


def align_items(ppg, lengths, phonemes, phoneme_lengths, want_gop=True, optional=None):
    """Forced alignment of item b = ppg[b, :, :lengths[b]] to phonemes[b, :phoneme_lengths[b]] (ppg_align):
    (items, 40, frames) on a GPU, phonemes a padded (items, max_phonemes) integer tensor, both lengths as host
    integers -> total (items,) fp32, starts (items, max_phonemes + 1) int32, score and gop (items, max_phonemes) fp32
    (gop None without want_gop).  Entries past an item's own N (N + 1 for starts) are zero.  With `optional`, a table
    of the shape of `phonemes` whose non-zero entries mark phonemes that may be left out, ppg_align_optional runs
    instead: a phoneme that was left out has starts[n] == starts[n + 1] and NaN for its score and gop."""
    x, lengths = _items(ppg, lengths, 'align')
    items, frames = x.shape[0], x.shape[2]
    device = x.device
    if phonemes.dim() != 2 or phonemes.shape[0] != items or not 1 <= phonemes.shape[1] <= ALIGN_MAX_PHONEMES:
        raise ValueError(
            f'phonemes must be ({items}, 1 to {ALIGN_MAX_PHONEMES}) for {items} items, got {tuple(phonemes.shape)}')
    table = phonemes.to(device=device, dtype=torch.int32).contiguous()
    most = table.shape[1]
    if optional is not None:
        if tuple(optional.shape) != tuple(table.shape):
            raise ValueError(f'optional must have the shape of phonemes {tuple(table.shape)}, got {tuple(optional.shape)}')
        optional = optional.to(device=device, dtype=torch.int32).contiguous()
    phoneme_lengths = [int(v) for v in phoneme_lengths]
    if len(phoneme_lengths) != items:
        raise ValueError(f'{len(phoneme_lengths)} phoneme lengths for {items} items')
    both = torch.tensor([lengths, phoneme_lengths], dtype=torch.int32).to(device)
    total = torch.empty((items,), dtype=torch.float32, device=device)
    starts = torch.zeros((items, most + 1), dtype=torch.int32, device=device)
    score = torch.zeros((items, most), dtype=torch.float32, device=device)
    gop = torch.zeros((items, most), dtype=torch.float32, device=device) if want_gop else None
    lib = library()
    bytes_for = lib.ppg_align_workspace_bytes if optional is None else lib.ppg_align_optional_workspace_bytes
    group = max(1, min(items, ALIGN_MAX_ITEMS, ALIGN_WORKSPACE_BYTES // bytes_for(1, frames, most)))
    size = bytes_for(group, frames, most)
    workspace = torch.empty((size,), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        for at in range(0, items, group):
            if optional is None:
                _check(lib.ppg_align(
                    device.index, x[at:].data_ptr(), frames, min(group, items - at), both[0, at:].data_ptr(),
                    table[at:].data_ptr(), most, both[1, at:].data_ptr(), total[at:].data_ptr(),
                    starts[at:].data_ptr(), score[at:].data_ptr(), gop[at:].data_ptr() if want_gop else None,
                    workspace.data_ptr(), size, stream))
            else:
                _check(lib.ppg_align_optional(
                    device.index, x[at:].data_ptr(), frames, min(group, items - at), both[0, at:].data_ptr(),
                    table[at:].data_ptr(), optional[at:].data_ptr(), most, both[1, at:].data_ptr(),
                    total[at:].data_ptr(), starts[at:].data_ptr(), score[at:].data_ptr(),
                    gop[at:].data_ptr() if want_gop else None, workspace.data_ptr(), size, stream))
    return total, starts, score, gop


def decode_items(ppg, lengths):
    """Run-length decode of item b = ppg[b, :, :lengths[b]] (ppg_decode): per frame the phoneme with the largest
    posterior, then runs of equal labels -> phonemes (items, frames) int32, starts (items, frames + 1) int32 and
    runs (items,) int32; entries past an item's runs (runs + 1 for starts) are zero."""
    x, lengths = _items(ppg, lengths, 'decode')
    items, frames = x.shape[0], x.shape[2]
    device = x.device
    lengths = torch.tensor(lengths, dtype=torch.int32).to(device)
    phonemes = torch.zeros((items, frames), dtype=torch.int32, device=device)
    starts = torch.zeros((items, frames + 1), dtype=torch.int32, device=device)
    runs = torch.empty((items,), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        for at in range(0, items, ALIGN_MAX_ITEMS):
            _check(library().ppg_decode(
                device.index, x[at:].data_ptr(), frames, min(ALIGN_MAX_ITEMS, items - at), lengths[at:].data_ptr(),
                phonemes[at:].data_ptr(), starts[at:].data_ptr(), runs[at:].data_ptr(), stream))
    return phonemes, starts, runs


RECOGNIZE_MAX_FRAMES = 262144    # PPG_RECOGNIZE_MAX_FRAMES
RECOGNIZE_MAX_ITEMS = 65535      # PPG_RECOGNIZE_MAX_ITEMS, per call of the library
RECOGNIZE_WORKSPACE_BYTES = 1 << 30  # a larger batch runs as several calls, each within this much workspace


def recognize_items(ppg, lengths, transitions, initial=None, final=None, want_gop=True):
    """Phoneme recognition of item b = ppg[b, :, :lengths[b]] (ppg_recognize): the best path through the 40 phonemes
    under `transitions` (40, 40) fp32, `initial` and `final` (40,) fp32 or None for zeros, all on the device of `ppg`
    and every entry finite or -inf (the caller's to check).  (items, 40, frames) on a GPU, lengths as host integers ->
    phonemes (items, frames) int32, starts (items, frames + 1) int32, runs (items,) int32, total (items,) fp32, score
    and gop (items, frames) fp32 (gop None without want_gop).  Entries past an item's runs (runs + 1 for starts) are
    zero; an item without a path has runs = 0 and total = -inf."""
    x, lengths = _items(ppg, lengths, 'recognize', RECOGNIZE_MAX_FRAMES)
    items, frames = x.shape[0], x.shape[2]
    device = x.device

    def weights(tensor, shape, name):
        if tensor is None:
            return None
        if not torch.is_tensor(tensor) or tuple(tensor.shape) != shape:
            raise ValueError(f'{name} must be a {shape} tensor, got {tuple(getattr(tensor, "shape", ()))}')
        return tensor.to(device=device, dtype=torch.float32).contiguous()
    transitions = weights(transitions, (40, 40), 'transitions')
    if transitions is None:
        raise ValueError('recognize takes a (40, 40) tensor of transitions')
    initial, final = weights(initial, (40,), 'initial'), weights(final, (40,), 'final')
    lengths = torch.tensor(lengths, dtype=torch.int32).to(device)
    phonemes = torch.zeros((items, frames), dtype=torch.int32, device=device)
    starts = torch.zeros((items, frames + 1), dtype=torch.int32, device=device)
    runs = torch.empty((items,), dtype=torch.int32, device=device)
    total = torch.empty((items,), dtype=torch.float32, device=device)
    score = torch.zeros((items, frames), dtype=torch.float32, device=device)
    gop = torch.zeros((items, frames), dtype=torch.float32, device=device) if want_gop else None
    lib = library()
    bytes_for = lib.ppg_recognize_workspace_bytes
    group = max(1, min(items, RECOGNIZE_MAX_ITEMS, RECOGNIZE_WORKSPACE_BYTES // bytes_for(1, frames)))
    size = bytes_for(group, frames)
    workspace = torch.empty((size,), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        for at in range(0, items, group):
            _check(lib.ppg_recognize(
                device.index, x[at:].data_ptr(), frames, min(group, items - at), lengths[at:].data_ptr(),
                transitions.data_ptr(), None if initial is None else initial.data_ptr(),
                None if final is None else final.data_ptr(), phonemes[at:].data_ptr(), starts[at:].data_ptr(),
                runs[at:].data_ptr(), total[at:].data_ptr(), score[at:].data_ptr(),
                gop[at:].data_ptr() if want_gop else None, workspace.data_ptr(), size, stream))
    return phonemes, starts, runs, total, score, gop


VITERBI_MAX_STATES = 1024        # PPG_VITERBI_MAX_STATES, per graph
VITERBI_MAX_ARCS = 32768         # PPG_VITERBI_MAX_ARCS, per graph
VITERBI_MAX_DEGREE = 255         # PPG_VITERBI_MAX_DEGREE: in-arcs of one state
VITERBI_MAX_FRAMES = 262144      # PPG_VITERBI_MAX_FRAMES
VITERBI_MAX_ITEMS = 65535        # PPG_VITERBI_MAX_ITEMS, per call of the library
VITERBI_MAX_GRAPHS = 65535       # PPG_VITERBI_MAX_GRAPHS, per call of the library
VITERBI_WORKSPACE_BYTES = 1 << 30  # a larger batch runs as several calls, each within this much workspace


def viterbi_items(ppg, lengths, state_begin, phonemes, stay, initial, final, arc_begin, sources, weights, which=None,
                  max_states=None, want_gop=True):
    """The best path of item b = ppg[b, :, :lengths[b]] through graph which[b] (ppg_viterbi).  The graphs travel
    packed, as the library takes them: state_begin (graphs + 1,), phonemes, stay, initial and final over all states,
    arc_begin (states + 1,), sources (counted inside each graph) and weights over all arcs; integer tensors become
    int32 and the weights fp32 on the device of `ppg`.  `which` holds a graph per item as host integers (None: graph 0
    for all); max_states bounds every graph's states (None: the library's limit or the number of states, whichever is
    less).  Nothing of the graphs is checked here: the device checks them, and an item whose graph it refuses, whose
    `which` names no graph or whose length is impossible has total NaN and runs 0.  (items, 40, frames) on a GPU ->
    states and phonemes (items, frames) int32, starts (items, frames + 1) int32, runs (items,) int32, total (items,)
    fp32, score and gop (items, frames) fp32 (gop None without want_gop).  Entries past an item's runs (runs + 1 for
    starts) are zero; an item without a path has runs = 0 and total = -inf."""
    x, lengths = _items(ppg, lengths, 'viterbi', VITERBI_MAX_FRAMES)
    items, frames = x.shape[0], x.shape[2]
    device = x.device

    def words(tensor, dtype, name):
        tensor = torch.as_tensor(tensor)
        if tensor.dim() != 1:
            raise ValueError(f'{name} must be one-dimensional, got {tuple(tensor.shape)}')
        return tensor.to(device=device, dtype=dtype).contiguous()
    state_begin, arc_begin = words(state_begin, torch.int32, 'state_begin'), words(arc_begin, torch.int32, 'arc_begin')
    phonemes, sources = words(phonemes, torch.int32, 'phonemes'), words(sources, torch.int32, 'sources')
    stay, initial = words(stay, torch.float32, 'stay'), words(initial, torch.float32, 'initial')
    final, weights = words(final, torch.float32, 'final'), words(weights, torch.float32, 'weights')
    graphs, count, arcs = state_begin.shape[0] - 1, phonemes.shape[0], sources.shape[0]
    if graphs < 1 or count < 1:
        raise ValueError('viterbi takes at least one graph of at least one state')
    for name, tensor, size in (('stay', stay, count), ('initial', initial, count), ('final', final, count),
                               ('arc_begin', arc_begin, count + 1), ('weights', weights, arcs)):
        if tensor.shape[0] != size:
            raise ValueError(f'{name} has {tensor.shape[0]} entries, {size} expected')
    if max_states is None:
        max_states = min(VITERBI_MAX_STATES, count)
    if which is not None:
        which = [int(v) for v in which]
        if len(which) != items:
            raise ValueError(f'{len(which)} graphs named for {items} items')
        which = torch.tensor(which, dtype=torch.int32).to(device)
    lengths = torch.tensor(lengths, dtype=torch.int32).to(device)
    states = torch.zeros((items, frames), dtype=torch.int32, device=device)
    labels = torch.zeros((items, frames), dtype=torch.int32, device=device)
    starts = torch.zeros((items, frames + 1), dtype=torch.int32, device=device)
    runs = torch.empty((items,), dtype=torch.int32, device=device)
    total = torch.empty((items,), dtype=torch.float32, device=device)
    score = torch.zeros((items, frames), dtype=torch.float32, device=device)
    gop = torch.zeros((items, frames), dtype=torch.float32, device=device) if want_gop else None
    lib = library()
    bytes_for = lib.ppg_viterbi_workspace_bytes
    one = bytes_for(1, frames, max_states)
    if one == 0:
        raise ValueError(f'viterbi takes graphs of 1 to {VITERBI_MAX_STATES} states, got max_states = {max_states}')
    group = max(1, min(items, VITERBI_MAX_ITEMS, VITERBI_WORKSPACE_BYTES // one))
    size = bytes_for(group, frames, max_states)
    workspace = torch.empty((size,), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        for at in range(0, items, group):
            _check(lib.ppg_viterbi(
                device.index, x[at:].data_ptr(), frames, min(group, items - at), lengths[at:].data_ptr(), graphs, count,
                arcs, max_states, state_begin.data_ptr(), phonemes.data_ptr(), stay.data_ptr(), initial.data_ptr(),
                final.data_ptr(), arc_begin.data_ptr(), sources.data_ptr() if arcs else None,
                weights.data_ptr() if arcs else None, None if which is None else which[at:].data_ptr(),
                states[at:].data_ptr(), labels[at:].data_ptr(), starts[at:].data_ptr(), runs[at:].data_ptr(),
                total[at:].data_ptr(), score[at:].data_ptr(), gop[at:].data_ptr() if want_gop else None,
                workspace.data_ptr(), size, stream))
    return states, labels, starts, runs, total, score, gop


POSTERIOR_MAX_FRAMES = 65536     # PPG_POSTERIOR_MAX_FRAMES
POSTERIOR_WORKSPACE_BYTES = 1 << 30  # a larger batch runs as several calls, each within this much workspace


def posterior_items(ppg, lengths, state_begin, phonemes, stay, initial, final, arc_begin, sources, weights, out_begin,
                    targets, out_weights, which=None, max_states=None, want_states=False):
    """The sum over all paths of item b = ppg[b, :, :lengths[b]] through graph which[b] (ppg_posterior).  The graphs
    travel packed as `viterbi_items` takes them, with their out-arc lists beside the in-arc lists: out_begin
    (states + 1,), targets (counted inside each graph) and out_weights over all arcs, the transpose of the in lists.
    Nothing of the graphs is checked here: the device checks them, and an item whose graph it refuses, whose `which`
    names no graph or whose length is impossible has total NaN.  (items, 40, frames) on a GPU -> total (items,)
    float64, the phoneme posterior (items, 40, frames) fp32 and the state occupancy (items, frames, max_states) fp32
    (None without want_states).  Frames past an item's length, states past its graph's, and the items without a path
    (total -inf) or refused (NaN) are zero."""
    x, lengths = _items(ppg, lengths, 'posterior', POSTERIOR_MAX_FRAMES)
    items, frames = x.shape[0], x.shape[2]
    device = x.device

    def words(tensor, dtype, name):
        tensor = torch.as_tensor(tensor)
        if tensor.dim() != 1:
            raise ValueError(f'{name} must be one-dimensional, got {tuple(tensor.shape)}')
        return tensor.to(device=device, dtype=dtype).contiguous()
    state_begin, arc_begin = words(state_begin, torch.int32, 'state_begin'), words(arc_begin, torch.int32, 'arc_begin')
    phonemes, sources = words(phonemes, torch.int32, 'phonemes'), words(sources, torch.int32, 'sources')
    stay, initial = words(stay, torch.float32, 'stay'), words(initial, torch.float32, 'initial')
    final, weights = words(final, torch.float32, 'final'), words(weights, torch.float32, 'weights')
    out_begin, targets = words(out_begin, torch.int32, 'out_begin'), words(targets, torch.int32, 'targets')
    out_weights = words(out_weights, torch.float32, 'out_weights')
    graphs, count, arcs = state_begin.shape[0] - 1, phonemes.shape[0], sources.shape[0]
    if graphs < 1 or count < 1:
        raise ValueError('posterior takes at least one graph of at least one state')
    for name, tensor, size in (('stay', stay, count), ('initial', initial, count), ('final', final, count),
                               ('arc_begin', arc_begin, count + 1), ('weights', weights, arcs),
                               ('out_begin', out_begin, count + 1), ('targets', targets, arcs),
                               ('out_weights', out_weights, arcs)):
        if tensor.shape[0] != size:
            raise ValueError(f'{name} has {tensor.shape[0]} entries, {size} expected')
    if max_states is None:
        max_states = min(VITERBI_MAX_STATES, count)
    if which is not None:
        which = [int(v) for v in which]
        if len(which) != items:
            raise ValueError(f'{len(which)} graphs named for {items} items')
        which = torch.tensor(which, dtype=torch.int32).to(device)
    lengths = torch.tensor(lengths, dtype=torch.int32).to(device)
    lib = library()
    bytes_for = lib.ppg_posterior_workspace_bytes
    one = bytes_for(1, frames, max_states)
    if one == 0:
        raise ValueError(f'posterior takes graphs of 1 to {VITERBI_MAX_STATES} states, got max_states = {max_states}')
    total = torch.empty((items,), dtype=torch.float64, device=device)
    post = torch.zeros((items, 40, frames), dtype=torch.float32, device=device)
    states = torch.zeros((items, frames, max_states), dtype=torch.float32, device=device) if want_states else None
    group = max(1, min(items, VITERBI_MAX_ITEMS, POSTERIOR_WORKSPACE_BYTES // one))
    size = bytes_for(group, frames, max_states)
    workspace = torch.empty((size,), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        for at in range(0, items, group):
            _check(lib.ppg_posterior(
                device.index, x[at:].data_ptr(), frames, min(group, items - at), lengths[at:].data_ptr(), graphs, count,
                arcs, max_states, state_begin.data_ptr(), phonemes.data_ptr(), stay.data_ptr(), initial.data_ptr(),
                final.data_ptr(), arc_begin.data_ptr(), sources.data_ptr() if arcs else None,
                weights.data_ptr() if arcs else None, out_begin.data_ptr(), targets.data_ptr() if arcs else None,
                out_weights.data_ptr() if arcs else None, None if which is None else which[at:].data_ptr(),
                total[at:].data_ptr(), post[at:].data_ptr(), states[at:].data_ptr() if want_states else None,
                max_states, workspace.data_ptr(), size, stream))
    return total, post, states


SEARCH_MAX_FRAMES = 262144       # PPG_SEARCH_MAX_FRAMES
SEARCH_MAX_PHONEMES = 256        # PPG_SEARCH_MAX_PHONEMES
SEARCH_MAX_HITS = 64             # PPG_SEARCH_MAX_HITS
SEARCH_MAX_ITEMS = 65535         # PPG_SEARCH_MAX_ITEMS, per call of the library
SEARCH_MAX_QUERIES = 65535       # PPG_SEARCH_MAX_QUERIES, per call of the library
SEARCH_WORKSPACE_BYTES = 1 << 30  # a larger batch runs as several calls, each within this much workspace


def search_items(ppg, lengths, table, counts, top=1, threshold=-math.inf, want_curve=False):
    """Phrase search (ppg_search): every query table[q, :counts[q]] in every recording ppg[b, :, :lengths[b]].
    (items, 40, frames) on a GPU, table a padded (queries, max_phonemes) integer tensor, both lengths as host
    integers -> begin, end (items, queries, top) int32, total, mean (items, queries, top) fp32, count (items, queries)
    int32, and the curve: None, or (curve_total fp32, curve_begin int32), each (items, queries, frames) with -inf and
    -1 at and past an item's own length.  Entries at or past count are -1, -1, NaN, NaN; a pair that cannot be searched
    has count -1."""
    if not ppg.is_cuda:
        raise PpgError('ppgs_amd: the post-ops work on HIP device tensors')
    x = ppg.to(torch.float32).contiguous()
    if x.dim() != 3 or x.shape[1] != 40 or x.shape[0] < 1:
        raise ValueError(f'PPGs must be (items >= 1, 40, frames), got {tuple(x.shape)}')
    items, frames = x.shape[0], x.shape[2]
    if not 1 <= frames <= SEARCH_MAX_FRAMES:
        raise ValueError(f'search takes 1 to {SEARCH_MAX_FRAMES} frames, got {frames}')
    lengths = [int(v) for v in lengths]
    if len(lengths) != items:
        raise ValueError(f'{len(lengths)} lengths for {items} items')
    device = x.device
    if table.dim() != 2 or table.shape[0] < 1 or not 1 <= table.shape[1] <= SEARCH_MAX_PHONEMES:
        raise ValueError(f'queries must be (queries >= 1, 1 to {SEARCH_MAX_PHONEMES}), got {tuple(table.shape)}')
    table = table.to(device=device, dtype=torch.int32).contiguous()
    queries, most = table.shape
    counts = [int(v) for v in counts]
    if len(counts) != queries:
        raise ValueError(f'{len(counts)} phoneme lengths for {queries} queries')
    top, threshold = int(top), float(threshold)
    if not 1 <= top <= SEARCH_MAX_HITS:
        raise ValueError(f'top must be 1 to {SEARCH_MAX_HITS}, got {top}')
    if threshold != threshold:
        raise ValueError('the threshold is NaN')
    lengths = torch.tensor(lengths, dtype=torch.int32).to(device)
    counts = torch.tensor(counts, dtype=torch.int32).to(device)
    shape = (items, queries, top)
    begin = torch.empty(shape, dtype=torch.int32, device=device)
    end = torch.empty(shape, dtype=torch.int32, device=device)
    total = torch.empty(shape, dtype=torch.float32, device=device)
    mean = torch.empty(shape, dtype=torch.float32, device=device)
    count = torch.empty((items, queries), dtype=torch.int32, device=device)
    curve = None
    if want_curve:
        curve = (torch.full((items, queries, frames), -math.inf, dtype=torch.float32, device=device),
                 torch.full((items, queries, frames), -1, dtype=torch.int32, device=device))
    lib = library()
    bytes_for = lib.ppg_search_workspace_bytes
    # queries per call: the prepared frames of one recording and as many curves as the budget holds; then recordings
    some = max(1, min(queries, SEARCH_MAX_QUERIES, (SEARCH_WORKSPACE_BYTES // frames - 176) // 8))
    group = max(1, min(items, SEARCH_MAX_ITEMS, SEARCH_WORKSPACE_BYTES // bytes_for(1, frames, some)))
    size = bytes_for(group, frames, some)
    workspace = torch.empty((size,), dtype=torch.uint8, device=device)
    outputs = (begin, end, total, mean, count) + (curve or ())

    def pointer(tensor):
        return tensor.data_ptr() if tensor is not None else None
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        for at in range(0, items, group):
            rows = min(group, items - at)
            for low in range(0, queries, some):
                columns = min(some, queries - low)
                if columns == queries:                          # the whole table: straight into the outputs
                    parts = [out[at:] for out in outputs]
                else:
                    parts = [out[at:at + rows, low:low + columns].contiguous() for out in outputs]
                slots = parts + [None] * (7 - len(parts))          # no curve: two NULL pointers
                _check(lib.ppg_search(
                    device.index, x[at:].data_ptr(), frames, rows, lengths[at:].data_ptr(), table[low:].data_ptr(),
                    most, columns, counts[low:].data_ptr(), top, threshold, *[pointer(part) for part in slots],
                    workspace.data_ptr(), size, stream))
                if columns != queries:
                    for out, part in zip(outputs, parts):
                        out[at:at + rows, low:low + columns].copy_(part)
    return begin, end, total, mean, count, curve


SEARCH_GRAPH_MAX_STATES = 256    # PPG_SEARCH_GRAPH_MAX_STATES, per graph
SEARCH_GRAPH_MAX_ARCS = 4096     # PPG_SEARCH_GRAPH_MAX_ARCS, per graph
SEARCH_GRAPH_MAX_GRAPHS = 65535  # = PPG_SEARCH_MAX_QUERIES, per call of the library
SEARCH_GRAPH_WORKSPACE_BYTES = 1 << 30  # a larger batch runs as several calls, each within this much workspace


def search_graph_items(ppg, lengths, state_begin, phonemes, stay, initial, final, arc_begin, sources, weights, top=1,
                       threshold=-math.inf, want_curve=False, max_states=None,
                       workspace_bytes=SEARCH_GRAPH_WORKSPACE_BYTES):
    """Phrase search over graphs (ppg_search_graph): every graph in every recording ppg[b, :, :lengths[b]].  The graphs
    travel packed as `viterbi_items` takes them; state_begin and arc_begin are host integers or CPU tensors (a batch
    that is split needs their values here).  Nothing of the graphs is checked: the device checks them, and a pair
    whose graph it refuses, whose graph has more than SEARCH_GRAPH_MAX_STATES states or SEARCH_GRAPH_MAX_ARCS arcs, or
    whose length is impossible has count -1.  max_states bounds every graph's states for the device's check (None: the
    library's limit or the number of states, whichever is less).  A batch that needs more than `workspace_bytes` runs
    as several calls: graphs in groups beside one recording's prepared frames, then recordings in groups.  The outputs
    are `search_items`' with the graphs in the place of the queries.  Nothing here waits for the device."""
    if not ppg.is_cuda:
        raise PpgError('ppgs_amd: the post-ops work on HIP device tensors')
    x = ppg.to(torch.float32).contiguous()
    if x.dim() != 3 or x.shape[1] != 40 or x.shape[0] < 1:
        raise ValueError(f'PPGs must be (items >= 1, 40, frames), got {tuple(x.shape)}')
    items, frames = x.shape[0], x.shape[2]
    if not 1 <= frames <= SEARCH_MAX_FRAMES:
        raise ValueError(f'search_graph takes 1 to {SEARCH_MAX_FRAMES} frames, got {frames}')
    lengths = [int(v) for v in lengths]
    if len(lengths) != items:
        raise ValueError(f'{len(lengths)} lengths for {items} items')
    device = x.device
    host = {'state_begin': torch.as_tensor(state_begin), 'arc_begin': torch.as_tensor(arc_begin)}

    def words(tensor, dtype, name):
        tensor = torch.as_tensor(tensor)
        if tensor.dim() != 1:
            raise ValueError(f'{name} must be one-dimensional, got {tuple(tensor.shape)}')
        return tensor.to(device=device, dtype=dtype).contiguous()
    state_begin, arc_begin = (words(host[name], torch.int32, name) for name in ('state_begin', 'arc_begin'))
    phonemes, sources = words(phonemes, torch.int32, 'phonemes'), words(sources, torch.int32, 'sources')
    stay, initial = words(stay, torch.float32, 'stay'), words(initial, torch.float32, 'initial')
    final, weights = words(final, torch.float32, 'final'), words(weights, torch.float32, 'weights')
    graphs, count, arcs = state_begin.shape[0] - 1, phonemes.shape[0], sources.shape[0]
    if graphs < 1 or count < 1:
        raise ValueError('search_graph takes at least one graph of at least one state')
    for name, tensor, size in (('stay', stay, count), ('initial', initial, count), ('final', final, count),
                               ('arc_begin', arc_begin, count + 1), ('weights', weights, arcs)):
        if tensor.shape[0] != size:
            raise ValueError(f'{name} has {tensor.shape[0]} entries, {size} expected')
    if max_states is None:
        max_states = min(VITERBI_MAX_STATES, count)
    if not 1 <= max_states <= VITERBI_MAX_STATES:
        raise ValueError(f'search_graph takes max_states from 1 to {VITERBI_MAX_STATES}, got {max_states}')
    top, threshold = int(top), float(threshold)
    if not 1 <= top <= SEARCH_MAX_HITS:
        raise ValueError(f'top must be 1 to {SEARCH_MAX_HITS}, got {top}')
    if threshold != threshold:
        raise ValueError('the threshold is NaN')
    lengths = torch.tensor(lengths, dtype=torch.int32).to(device)
    shape = (items, graphs, top)
    begin = torch.empty(shape, dtype=torch.int32, device=device)
    end = torch.empty(shape, dtype=torch.int32, device=device)
    total = torch.empty(shape, dtype=torch.float32, device=device)
    mean = torch.empty(shape, dtype=torch.float32, device=device)
    hits = torch.empty((items, graphs), dtype=torch.int32, device=device)
    curve = None
    if want_curve:
        curve = (torch.full((items, graphs, frames), -math.inf, dtype=torch.float32, device=device),
                 torch.full((items, graphs, frames), -1, dtype=torch.int32, device=device))
    lib = library()
    bytes_for = lib.ppg_search_graph_workspace_bytes
    # graphs per call: one recording's prepared frames (176 bytes a frame), 8 bytes per pair and frame of curve, 8 per
    # graph of verdict and ones, five blocks rounded up to 256 bytes; then recordings
    some = max(1, min(graphs, SEARCH_GRAPH_MAX_GRAPHS, (int(workspace_bytes) - 1280 - 176 * frames) // (8 * frames + 8)))
    group = max(1, min(items, SEARCH_MAX_ITEMS, int(workspace_bytes) // bytes_for(1, frames, some)))
    size = bytes_for(group, frames, some)
    workspace = torch.empty((size,), dtype=torch.uint8, device=device)
    outputs = (begin, end, total, mean, hits) + (curve or ())
    if some < graphs:                                           # the packed graphs of a group count from its own first
        first_state, first_arc = host['state_begin'].tolist(), host['arc_begin'].tolist()

    def pointer(tensor):
        return tensor.data_ptr() if tensor is not None else None
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        for at in range(0, items, group):
            rows = min(group, items - at)
            for low in range(0, graphs, some):
                columns = min(some, graphs - low)
                if columns == graphs:                           # every graph: straight into the outputs
                    parts = [out[at:] for out in outputs]
                    s0, s1, a0, a1 = 0, count, 0, arcs
                    state_part, arc_part = state_begin, arc_begin
                else:
                    parts = [out[at:at + rows, low:low + columns].contiguous() for out in outputs]
                    s0, s1 = first_state[low], first_state[low + columns]
                    a0, a1 = first_arc[s0], first_arc[s1]
                    state_part = (state_begin[low:low + columns + 1] - s0).contiguous()
                    arc_part = (arc_begin[s0:s1 + 1] - a0).contiguous()
                slots = parts + [None] * (7 - len(parts))          # no curve: two NULL pointers
                _check(lib.ppg_search_graph(
                    device.index, x[at:].data_ptr(), frames, rows, lengths[at:].data_ptr(), columns, s1 - s0, a1 - a0,
                    max_states, state_part.data_ptr(), phonemes[s0:].data_ptr(), stay[s0:].data_ptr(),
                    initial[s0:].data_ptr(), final[s0:].data_ptr(), arc_part.data_ptr(),
                    sources[a0:].data_ptr() if a1 > a0 else None, weights[a0:].data_ptr() if a1 > a0 else None, top,
                    threshold, *[pointer(part) for part in slots], workspace.data_ptr(), size, stream))
                if columns != graphs:
                    for out, part in zip(outputs, parts):
                        out[at:at + rows, low:low + columns].copy_(part)
    return begin, end, total, mean, hits, curve


def search_stream_state(device, streams, queries, most):
    """The device block of a live search (ppg_search_stream_*), reset: `streams` streams x `queries` queries of at most
    `most` phonemes.  uint8; its owner passes it to the three calls below with the same three numbers."""
    size = library().ppg_search_stream_state_bytes(streams, queries, most)
    if size == 0:
        raise ValueError(f'a live search takes 1 to {SEARCH_MAX_ITEMS} streams, 1 to {SEARCH_MAX_QUERIES} queries and 1 to '
                         f'{SEARCH_MAX_PHONEMES} phonemes, got {streams}, {queries} and {most}')
    state = torch.empty((size,), dtype=torch.uint8, device=device)
    search_stream_reset(state, streams, queries, most)
    return state


def search_stream_reset(state, streams, queries, most, which=None):
    """ppg_search_stream_reset on the current stream: `which` is None (all) or a device int32 (streams,) of flags."""
    with torch.cuda.device(state.device):
        _check(library().ppg_search_stream_reset(
            state.device.index, state.data_ptr(), streams, queries, most,
            which.data_ptr() if which is not None else None, torch.cuda.current_stream().cuda_stream))


def search_stream_push(state, ppg, lengths, table, counts, threshold, patience, cap, workspace, want_curve=False):
    """ppg_search_stream_push on the current stream: ppg (streams, 40, frames) fp32, lengths (streams,) and counts
    (queries,) int32, table (queries, most) int32, all contiguous on the state's device; workspace a uint8 tensor
    there -> begin, end (streams, queries, cap) int32, total, mean fp32, count (streams, queries) int32 and the curve of
    the pushed frames: None, or (curve_total fp32, curve_begin int32), each (streams, queries, frames) with -inf and
    -1 at and past a stream's own length."""
    device = state.device
    streams, frames = ppg.shape[0], ppg.shape[2]
    queries, most = table.shape
    shape = (streams, queries, cap)
    begin = torch.empty(shape, dtype=torch.int32, device=device)
    end = torch.empty(shape, dtype=torch.int32, device=device)
    total = torch.empty(shape, dtype=torch.float32, device=device)
    mean = torch.empty(shape, dtype=torch.float32, device=device)
    count = torch.empty((streams, queries), dtype=torch.int32, device=device)
    curve = None
    if want_curve:
        curve = (torch.full((streams, queries, frames), -math.inf, dtype=torch.float32, device=device),
                 torch.full((streams, queries, frames), -1, dtype=torch.int32, device=device))
    with torch.cuda.device(device):
        _check(library().ppg_search_stream_push(
            device.index, state.data_ptr(), ppg.data_ptr(), frames, streams, lengths.data_ptr(), table.data_ptr(), most,
            queries, counts.data_ptr(), threshold, patience, cap, begin.data_ptr(), end.data_ptr(), total.data_ptr(),
            mean.data_ptr(), count.data_ptr(), curve[0].data_ptr() if curve else None,
            curve[1].data_ptr() if curve else None, workspace.data_ptr(), workspace.numel(),
            torch.cuda.current_stream().cuda_stream))
    return begin, end, total, mean, count, curve


def search_stream_flush(state, streams, queries, most, which=None):
    """ppg_search_stream_flush on the current stream -> begin, end int32, total, mean fp32 (streams, queries, 1) and
    count (streams, queries) int32: 1 where a hit was pending."""
    device = state.device
    begin = torch.empty((streams, queries, 1), dtype=torch.int32, device=device)
    end = torch.empty((streams, queries, 1), dtype=torch.int32, device=device)
    total = torch.empty((streams, queries, 1), dtype=torch.float32, device=device)
    mean = torch.empty((streams, queries, 1), dtype=torch.float32, device=device)
    count = torch.empty((streams, queries), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _check(library().ppg_search_stream_flush(
            device.index, state.data_ptr(), streams, queries, most, which.data_ptr() if which is not None else None,
            begin.data_ptr(), end.data_ptr(), total.data_ptr(), mean.data_ptr(), count.data_ptr(),
            torch.cuda.current_stream().cuda_stream))
    return begin, end, total, mean, count


def search_graph_stream_state(device, streams, packed):
    """The device block of a live search over graphs (ppg_search_graph_stream_*), opened: `streams` streams x the
    graphs of `packed` (a PackedGraphs of contiguous int32 / fp32 tensors on `device`, as the live Viterbi takes it).
    uint8; its owner passes it to the calls below with the same numbers and the same `packed`."""
    size = library().ppg_search_graph_stream_state_bytes(streams, packed.graphs, packed.max_states)
    if size == 0:
        raise ValueError(f'a live search over graphs takes 1 to {SEARCH_MAX_ITEMS} streams, 1 to '
                         f'{SEARCH_GRAPH_MAX_GRAPHS} graphs and 1 to {VITERBI_MAX_STATES} states, got {streams}, '
                         f'{packed.graphs} and {packed.max_states}')
    state = torch.empty((size,), dtype=torch.uint8, device=device)
    search_graph_stream_open(state, streams, packed)
    return state


def search_graph_stream_open(state, streams, packed):
    """ppg_search_graph_stream_open on the current stream: the device checks the graphs, keeps its verdicts in the
    state, and every stream starts at frame 0."""
    with torch.cuda.device(state.device):
        _check(library().ppg_search_graph_stream_open(
            state.device.index, state.data_ptr(), streams, *_graph_arguments(packed),
            torch.cuda.current_stream().cuda_stream))


def search_graph_stream_reset(state, streams, graphs, max_states, which=None):
    """ppg_search_graph_stream_reset on the current stream: `which` is None (all) or a device int32 (streams,) of
    flags."""
    with torch.cuda.device(state.device):
        _check(library().ppg_search_graph_stream_reset(
            state.device.index, state.data_ptr(), streams, graphs, max_states,
            which.data_ptr() if which is not None else None, torch.cuda.current_stream().cuda_stream))


def search_graph_stream_push(state, ppg, lengths, packed, threshold, patience, cap, workspace, want_curve=False):
    """ppg_search_graph_stream_push on the current stream: ppg (streams, 40, frames) fp32 and lengths (streams,) int32,
    contiguous on the state's device; `packed` the graphs the state was opened with; workspace a uint8 tensor there ->
    the outputs of search_stream_push with the graphs in the place of the queries."""
    device = state.device
    streams, frames = ppg.shape[0], ppg.shape[2]
    shape = (streams, packed.graphs, cap)
    begin = torch.empty(shape, dtype=torch.int32, device=device)
    end = torch.empty(shape, dtype=torch.int32, device=device)
    total = torch.empty(shape, dtype=torch.float32, device=device)
    mean = torch.empty(shape, dtype=torch.float32, device=device)
    count = torch.empty((streams, packed.graphs), dtype=torch.int32, device=device)
    curve = None
    if want_curve:
        curve = (torch.full((streams, packed.graphs, frames), -math.inf, dtype=torch.float32, device=device),
                 torch.full((streams, packed.graphs, frames), -1, dtype=torch.int32, device=device))
    with torch.cuda.device(device):
        _check(library().ppg_search_graph_stream_push(
            device.index, state.data_ptr(), ppg.data_ptr(), frames, streams, lengths.data_ptr(),
            *_graph_arguments(packed), threshold, patience, cap, begin.data_ptr(), end.data_ptr(), total.data_ptr(),
            mean.data_ptr(), count.data_ptr(), curve[0].data_ptr() if curve else None,
            curve[1].data_ptr() if curve else None, workspace.data_ptr(), workspace.numel(),
            torch.cuda.current_stream().cuda_stream))
    return begin, end, total, mean, count, curve


def search_graph_stream_flush(state, streams, graphs, max_states, which=None):
    """ppg_search_graph_stream_flush on the current stream -> begin, end int32, total, mean fp32 (streams, graphs, 1)
    and count (streams, graphs) int32: 1 where a hit was pending."""
    device = state.device
    begin = torch.empty((streams, graphs, 1), dtype=torch.int32, device=device)
    end = torch.empty((streams, graphs, 1), dtype=torch.int32, device=device)
    total = torch.empty((streams, graphs, 1), dtype=torch.float32, device=device)
    mean = torch.empty((streams, graphs, 1), dtype=torch.float32, device=device)
    count = torch.empty((streams, graphs), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _check(library().ppg_search_graph_stream_flush(
            device.index, state.data_ptr(), streams, graphs, max_states,
            which.data_ptr() if which is not None else None, begin.data_ptr(), end.data_ptr(), total.data_ptr(),
            mean.data_ptr(), count.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return begin, end, total, mean, count


RECOGNIZE_STREAM_MIN_WINDOW = 64     # PPG_RECOGNIZE_STREAM_MIN_WINDOW
RECOGNIZE_STREAM_MAX_WINDOW = 65536  # PPG_RECOGNIZE_STREAM_MAX_WINDOW
RECOGNIZE_STREAM_MAX_STREAMS = 65535  # PPG_RECOGNIZE_STREAM_MAX_STREAMS


def recognize_stream_state(device, streams, window):
    """The device block of a live recogniser (ppg_recognize_stream_*), reset: `streams` streams with a ring of `window`
    frames each.  uint8; its owner passes it to the three calls below with the same two numbers."""
    size = library().ppg_recognize_stream_state_bytes(streams, window)
    if size == 0:
        raise ValueError(f'a live recogniser takes 1 to {RECOGNIZE_STREAM_MAX_STREAMS} streams and a window that is a '
                         f'multiple of 64 from {RECOGNIZE_STREAM_MIN_WINDOW} to {RECOGNIZE_STREAM_MAX_WINDOW}, got '
                         f'{streams} and {window}')
    state = torch.empty((size,), dtype=torch.uint8, device=device)
    recognize_stream_reset(state, streams, window)
    return state


def recognize_stream_reset(state, streams, window, which=None):
    """ppg_recognize_stream_reset on the current stream: `which` is None (all) or a device int32 (streams,) of flags."""
    with torch.cuda.device(state.device):
        _check(library().ppg_recognize_stream_reset(
            state.device.index, state.data_ptr(), streams, window, which.data_ptr() if which is not None else None,
            torch.cuda.current_stream().cuda_stream))


def _run_outputs(device, streams, cap, want_gop):
    return (torch.empty((streams, cap), dtype=torch.int32, device=device),
            torch.empty((streams, cap), dtype=torch.int32, device=device),
            torch.empty((streams, cap), dtype=torch.int32, device=device),
            torch.empty((streams, cap), dtype=torch.float32, device=device),
            torch.empty((streams, cap), dtype=torch.float32, device=device) if want_gop else None,
            torch.empty((streams,), dtype=torch.int32, device=device))


def recognize_stream_push(state, window, ppg, lengths, transitions, initial, max_lag, cap, workspace, want_gop=True):
    """ppg_recognize_stream_push on the current stream: ppg (streams, 40, frames) fp32, lengths (streams,) int32,
    transitions (40, 40) and initial (40,) or None fp32, all contiguous on the state's device; workspace a uint8 tensor
    there -> phonemes, begin, end (streams, cap) int32, score, gop (streams, cap) fp32 (gop None without want_gop) and
    count (streams,) int32: the runs closed in this push; slots at or past it are -1 / NaN."""
    device = state.device
    streams, frames = ppg.shape[0], ppg.shape[2]
    phonemes, begin, end, score, gop, count = _run_outputs(device, streams, cap, want_gop)
    with torch.cuda.device(device):
        _check(library().ppg_recognize_stream_push(
            device.index, state.data_ptr(), streams, window, ppg.data_ptr(), frames, lengths.data_ptr(),
            transitions.data_ptr(), initial.data_ptr() if initial is not None else None, max_lag, cap,
            phonemes.data_ptr(), begin.data_ptr(), end.data_ptr(), score.data_ptr(),
            gop.data_ptr() if want_gop else None, count.data_ptr(), workspace.data_ptr(), workspace.numel(),
            torch.cuda.current_stream().cuda_stream))
    return phonemes, begin, end, score, gop, count


def recognize_stream_flush(state, streams, window, final, cap, which=None, want_gop=True):
    """ppg_recognize_stream_flush on the current stream -> the run outputs of recognize_stream_push, and total fp32 and
    forced int32 (streams,)."""
    device = state.device
    phonemes, begin, end, score, gop, count = _run_outputs(device, streams, cap, want_gop)
    total = torch.empty((streams,), dtype=torch.float32, device=device)
    forced = torch.empty((streams,), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _check(library().ppg_recognize_stream_flush(
            device.index, state.data_ptr(), streams, window, final.data_ptr() if final is not None else None,
            which.data_ptr() if which is not None else None, cap, phonemes.data_ptr(), begin.data_ptr(),
            end.data_ptr(), score.data_ptr(), gop.data_ptr() if want_gop else None, count.data_ptr(),
            total.data_ptr(), forced.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return phonemes, begin, end, score, gop, count, total, forced


VITERBI_STREAM_MIN_WINDOW = 64       # PPG_VITERBI_STREAM_MIN_WINDOW
VITERBI_STREAM_MAX_WINDOW = 65536    # PPG_VITERBI_STREAM_MAX_WINDOW
VITERBI_STREAM_MAX_STREAMS = 65535   # PPG_VITERBI_STREAM_MAX_STREAMS

PackedGraphs = collections.namedtuple('PackedGraphs', [
    'graphs', 'states', 'arcs', 'max_states', 'state_begin', 'phonemes', 'stay', 'initial', 'final', 'arc_begin',
    'sources', 'weights'])


def _graph_arguments(packed):
    """The graph arguments of the ppg_viterbi_stream_* entries from a PackedGraphs of device tensors."""
    return (packed.graphs, packed.states, packed.arcs, packed.max_states, packed.state_begin.data_ptr(),
            packed.phonemes.data_ptr(), packed.stay.data_ptr(), packed.initial.data_ptr(), packed.final.data_ptr(),
            packed.arc_begin.data_ptr(), packed.sources.data_ptr() if packed.arcs else None,
            packed.weights.data_ptr() if packed.arcs else None)


def viterbi_stream_state(device, streams, window, packed, which=None):
    """The device block of a live Viterbi (ppg_viterbi_stream_*), opened: `streams` streams with a ring of `window`
    frames each over the graphs of `packed` (a PackedGraphs of contiguous int32 / fp32 tensors on `device`), stream i
    on graph which[i] (a device int32 tensor; None: graph 0).  uint8; its owner passes it to the calls below with the
    same numbers and the same `packed`."""
    size = library().ppg_viterbi_stream_state_bytes(streams, window, packed.max_states)
    if size == 0:
        raise ValueError(f'a live Viterbi takes 1 to {VITERBI_STREAM_MAX_STREAMS} streams, a window that is a multiple '
                         f'of 64 from {VITERBI_STREAM_MIN_WINDOW} to {VITERBI_STREAM_MAX_WINDOW} and graphs of 1 to '
                         f'{VITERBI_MAX_STATES} states, got {streams}, {window} and {packed.max_states}')
    state = torch.empty((size,), dtype=torch.uint8, device=device)
    viterbi_stream_open(state, streams, window, packed, which)
    return state


def viterbi_stream_open(state, streams, window, packed, which=None):
    """ppg_viterbi_stream_open on the current stream: the device checks the graphs and every stream starts at frame 0."""
    with torch.cuda.device(state.device):
        _check(library().ppg_viterbi_stream_open(
            state.device.index, state.data_ptr(), streams, window, *_graph_arguments(packed),
            which.data_ptr() if which is not None else None, torch.cuda.current_stream().cuda_stream))


def viterbi_stream_reset(state, streams, window, max_states, which=None):
    """ppg_viterbi_stream_reset on the current stream: `which` is None (all) or a device int32 (streams,) of flags."""
    with torch.cuda.device(state.device):
        _check(library().ppg_viterbi_stream_reset(
            state.device.index, state.data_ptr(), streams, window, max_states,
            which.data_ptr() if which is not None else None, torch.cuda.current_stream().cuda_stream))


def viterbi_stream_push(state, window, ppg, lengths, packed, max_lag, cap, workspace, want_gop=True):
    """ppg_viterbi_stream_push on the current stream: ppg (streams, 40, frames) fp32 and lengths (streams,) int32,
    contiguous on the state's device; `packed` the graphs the state was opened with; workspace a uint8 tensor there ->
    states, phonemes, begin, end (streams, cap) int32, score, gop (streams, cap) fp32 (gop None without want_gop) and
    count (streams,) int32: the runs closed in this push; slots at or past it are -1 / NaN."""
    device = state.device
    streams, frames = ppg.shape[0], ppg.shape[2]
    states = torch.empty((streams, cap), dtype=torch.int32, device=device)
    phonemes, begin, end, score, gop, count = _run_outputs(device, streams, cap, want_gop)
    with torch.cuda.device(device):
        _check(library().ppg_viterbi_stream_push(
            device.index, state.data_ptr(), streams, window, ppg.data_ptr(), frames, lengths.data_ptr(),
            *_graph_arguments(packed), max_lag, cap, states.data_ptr(), phonemes.data_ptr(), begin.data_ptr(),
            end.data_ptr(), score.data_ptr(), gop.data_ptr() if want_gop else None, count.data_ptr(),
            workspace.data_ptr(), workspace.numel(), torch.cuda.current_stream().cuda_stream))
    return states, phonemes, begin, end, score, gop, count


def viterbi_stream_flush(state, streams, window, packed, cap, which=None, want_gop=True):
    """ppg_viterbi_stream_flush on the current stream -> the run outputs of viterbi_stream_push, and total fp32 and
    forced int32 (streams,)."""
    device = state.device
    states = torch.empty((streams, cap), dtype=torch.int32, device=device)
    phonemes, begin, end, score, gop, count = _run_outputs(device, streams, cap, want_gop)
    total = torch.empty((streams,), dtype=torch.float32, device=device)
    forced = torch.empty((streams,), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _check(library().ppg_viterbi_stream_flush(
            device.index, state.data_ptr(), streams, window, *_graph_arguments(packed),
            which.data_ptr() if which is not None else None, cap, states.data_ptr(), phonemes.data_ptr(),
            begin.data_ptr(), end.data_ptr(), score.data_ptr(), gop.data_ptr() if want_gop else None,
            count.data_ptr(), total.data_ptr(), forced.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return states, phonemes, begin, end, score, gop, count, total, forced


POSTERIOR_STREAM_MAX_PUSH = 2 ** 26 - 1  # PPG_POSTERIOR_STREAM_MAX_PUSH: frames * streams of one push

PackedOutGraphs = collections.namedtuple('PackedOutGraphs', PackedGraphs._fields + ('out_begin', 'targets', 'out_weights'))


def _out_graph_arguments(packed):
    """The graph arguments of the ppg_posterior_stream_* entries from a PackedOutGraphs of device tensors."""
    return _graph_arguments(packed) + (
        packed.out_begin.data_ptr(), packed.targets.data_ptr() if packed.arcs else None,
        packed.out_weights.data_ptr() if packed.arcs else None)


def posterior_stream_state(device, streams, window, packed, block, lag, which=None):
    """The device block of a live posterior (ppg_posterior_stream_*), opened: `streams` streams with a ring of `window`
    frames each over the graphs of `packed` (a PackedOutGraphs of contiguous int32 / fp32 tensors on `device`), stream i
    on graph which[i] (a device int32 tensor; None: graph 0), blocks of `block` frames smoothed by `lag` more.  uint8;
    its owner passes it to the calls below with the same numbers and the same `packed`."""
    size = library().ppg_posterior_stream_state_bytes(streams, window, packed.max_states)
    if size == 0:
        raise ValueError(f'a live posterior takes 1 to {VITERBI_STREAM_MAX_STREAMS} streams, a window that is a '
                         f'multiple of 64 from {VITERBI_STREAM_MIN_WINDOW} to {VITERBI_STREAM_MAX_WINDOW} and graphs of '
                         f'1 to {VITERBI_MAX_STATES} states, got {streams}, {window} and {packed.max_states}')
    state = torch.empty((size,), dtype=torch.uint8, device=device)
    posterior_stream_open(state, streams, window, packed, block, lag, which)
    return state


def posterior_stream_open(state, streams, window, packed, block, lag, which=None):
    """ppg_posterior_stream_open on the current stream: the device checks the graphs and every stream starts at frame
    0."""
    with torch.cuda.device(state.device):
        _check(library().ppg_posterior_stream_open(
            state.device.index, state.data_ptr(), streams, window, *_out_graph_arguments(packed),
            which.data_ptr() if which is not None else None, block, lag, torch.cuda.current_stream().cuda_stream))


def posterior_stream_reset(state, streams, window, max_states, which=None):
    """ppg_posterior_stream_reset on the current stream: `which` is None (all) or a device int32 (streams,) of flags."""
    with torch.cuda.device(state.device):
        _check(library().ppg_posterior_stream_reset(
            state.device.index, state.data_ptr(), streams, window, max_states,
            which.data_ptr() if which is not None else None, torch.cuda.current_stream().cuda_stream))


def _posterior_outputs(device, streams, cap, max_states, want_states):
    post = torch.zeros((streams, 40, cap), dtype=torch.float32, device=device)
    states = torch.zeros((streams, cap, max_states), dtype=torch.float32, device=device) if want_states else None
    begin = torch.zeros((streams,), dtype=torch.int32, device=device)
    count = torch.zeros((streams,), dtype=torch.int32, device=device)
    float64 = torch.zeros((streams,), dtype=torch.float64, device=device)
    return post, states, begin, count, float64


def posterior_stream_push(state, window, ppg, lengths, packed, cap, workspace, want_states=False):
    """ppg_posterior_stream_push on the current stream: ppg (streams, 40, frames) fp32 and lengths (streams,) int32,
    contiguous on the state's device; `packed` the graphs the state was opened with; workspace a uint8 tensor there ->
    post (streams, 40, cap) fp32, the occupancy (streams, cap, max_states) fp32 (None without want_states), begin and
    count (streams,) int32 and evidence (streams,) float64.  Column j is frame begin + j; columns at or past count are
    zero."""
    device = state.device
    streams, frames = ppg.shape[0], ppg.shape[2]
    post, states, begin, count, evidence = _posterior_outputs(device, streams, cap, packed.max_states, want_states)
    with torch.cuda.device(device):
        _check(library().ppg_posterior_stream_push(
            device.index, state.data_ptr(), streams, window, ppg.data_ptr(), frames, lengths.data_ptr(),
            *_out_graph_arguments(packed), cap, post.data_ptr(), states.data_ptr() if want_states else None,
            packed.max_states, begin.data_ptr(), count.data_ptr(), evidence.data_ptr(), workspace.data_ptr(),
            workspace.numel(), torch.cuda.current_stream().cuda_stream))
    return post, states, begin, count, evidence


def posterior_stream_flush(state, streams, window, packed, cap, which=None, want_states=False):
    """ppg_posterior_stream_flush on the current stream -> the outputs of posterior_stream_push with total (streams,)
    float64 in the place of evidence."""
    device = state.device
    post, states, begin, count, total = _posterior_outputs(device, streams, cap, packed.max_states, want_states)
    with torch.cuda.device(device):
        _check(library().ppg_posterior_stream_flush(
            device.index, state.data_ptr(), streams, window, *_out_graph_arguments(packed),
            which.data_ptr() if which is not None else None, cap, post.data_ptr(),
            states.data_ptr() if want_states else None, packed.max_states, begin.data_ptr(), count.data_ptr(),
            total.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return post, states, begin, count, total


METRICS_FIXED_POINT = 2.0 ** 32        # the real-valued accumulators of PpgMetricsState count units of 2^-32


def metrics_fields(words):
    """PpgMetricsState as a dict, from its int64 words (numpy, length sizeof / 8): Python ints for the scalars,
    int64 arrays for the per-class counts and the two matrices.  Fixed-point fields stay integers (exact); divide
    by METRICS_FIXED_POINT for their value."""
    out, offset = {}, 0
    for name, kind in PpgMetricsState._fields_:
        size = ctypes.sizeof(kind) // 8
        if size == 1:
            out[name] = int(words[offset])
        elif size == 40:
            out[name] = words[offset:offset + size].copy()
        else:
            out[name] = words[offset:offset + size].reshape(40, 40).copy()
        offset += size
    del out['reserved']
    return out


class MetricsState:
    """Frame metrics accumulated on the GPU (ppg_metrics_update): update() is one kernel launch on the current
    stream and synchronises nothing; read() is the only place that does.  The state is a function of the multiset
    of (frame, label) pairs seen, bit for bit, however they were split over updates, streams or devices."""

    def __init__(self, device=0, k=3, similarity_mix=None, class_weights=None, loss_weights=None):
        if not torch.cuda.is_available():
            raise PpgError('ppgs_amd: no HIP device visible; the metrics have no CPU path')
        if not 1 <= int(k) <= 8:
            raise ValueError(f'top-k needs 1 <= k <= 8, got {k}')
        self._lib = library()
        self.device = torch.device('cuda', device) if isinstance(device, int) else torch.device(device)
        self.k = int(k)

        def table(tensor, shape):
            if tensor is None:
                return None
            tensor = torch.as_tensor(tensor).to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(tensor.shape) != shape:
                raise ValueError(f'expected a tensor of shape {shape}, got {tuple(tensor.shape)}')
            return tensor
        self.similarity_mix = table(similarity_mix, (40, 40))
        self.class_weights = table(class_weights, (40,))
        self.loss_weights = table(loss_weights, (40,))
        assert ctypes.sizeof(PpgMetricsState) == self._lib.ppg_metrics_state_bytes()
        self.state = torch.zeros(ctypes.sizeof(PpgMetricsState) // 8, dtype=torch.int64, device=self.device)

    def reset(self):
        with torch.cuda.device(self.device):
            _check(self._lib.ppg_metrics_reset(
                self.device.index, self.state.data_ptr(), torch.cuda.current_stream().cuda_stream))

    def _on_device(self, tensor, dtype=None):
        tensor = torch.as_tensor(tensor)
        if not tensor.is_cuda:            # a host tensor goes through pinned memory: the copy is asynchronous too
            tensor = tensor.contiguous().pin_memory()
        return tensor.to(device=self.device, dtype=dtype, non_blocking=True).contiguous()

    def update(self, logits, labels, lengths=None):
        """logits (batch, 40, frames) fp32 on this device, labels (batch, frames) int64 / int32 (-100: no label),
        lengths (batch,) or None.  Labels and lengths on the device are used where they lie."""
        if not (torch.is_tensor(logits) and logits.is_cuda and logits.device == self.device):
            raise PpgError('ppgs_amd: the metrics work on logits on their own HIP device')
        if logits.dim() != 3 or logits.shape[1] != 40:
            raise ValueError(f'logits must be (batch, 40, frames), got {tuple(logits.shape)}')
        logits = logits.to(torch.float32).contiguous()
        batch, _, frames = logits.shape
        labels = self._on_device(labels)
        if labels.dtype != torch.int32:
            labels = labels.to(torch.int64)
        if tuple(labels.shape) != (batch, frames):
            raise ValueError(f'labels must be ({batch}, {frames}), got {tuple(labels.shape)}')
        if lengths is not None:
            lengths = self._on_device(lengths, torch.int64).reshape(-1)
            if lengths.numel() != batch:
                raise ValueError(f'lengths has {lengths.numel()} entries for a batch of {batch}')

        def pointer(tensor):
            return tensor.data_ptr() if tensor is not None else None
        with torch.cuda.device(self.device):
            _check(self._lib.ppg_metrics_update(
                self.device.index, logits.data_ptr(), labels.data_ptr(), int(labels.dtype == torch.int64),
                pointer(lengths), batch, frames, self.k, pointer(self.similarity_mix), pointer(self.class_weights),
                pointer(self.loss_weights), self.state.data_ptr(), torch.cuda.current_stream().cuda_stream))
        if not torch.cuda.is_current_stream_capturing():
            for tensor in (logits, labels, lengths):  # updates on a side stream: the allocator must not reuse them early
                if tensor is not None:
                    tensor.record_stream(torch.cuda.current_stream(self.device))

    def read(self):
        """The state as a dict (metrics_fields) plus 'k'; synchronises with the device."""
        out = metrics_fields(self.state.cpu().numpy())
        out['k'] = self.k
        return out

    @staticmethod
    def merge(*reads):
        """Sum of read() dicts (several ranks or devices): integer addition, so exact."""
        out = dict(reads[0])
        for other in reads[1:]:
            if other['k'] != out['k']:
                raise ValueError('states with different k do not merge')
            for key, value in other.items():
                if key != 'k':
                    out[key] = out[key] + value
        return out


class PpgW2v2Weights(ctypes.Structure):
    _fields_ = [('conv_weight', _FP * 7), ('norm_weight', _FP), ('norm_bias', _FP)]


def audio_stream_frames(received, flushed=False):
    """Mel frames the incremental frontend has emitted after `received` samples of a recording
    (ppg_audio_stream_frames, host only): frame t needs samples up to 160 t + 591 and frames leave in the
    pairs (2 j, 2 j + 1) the transform works on, so ((received - 592) // 160 + 1) & ~1 while the recording
    goes on (0 below 592 samples) and received // 160 once it has ended."""
    return int(library().ppg_audio_stream_frames(int(received), int(bool(flushed))))


class FrontendStream:
    """The mel frontend for audio that arrives in pieces (include/ppgs_amd.h: ppg_frontend_stream_*): `batch`
    recordings, each handed its new 16 kHz samples push by push, each returning the mel frames that became
    computable -- the frames :func:`frontend` computes for the whole recording, bit for bit.  A frame needs 592
    samples past its start and leaves together with its pair partner (audio_stream_frames); flush ends a
    recording (its last frames take the reflection about the last sample; it must have more than 432 samples).
    Only the samples the next frames need stay on the device.  Pushes of one object must be ordered on the device
    (one HIP stream, or events between them).  16 kHz only: there is no streaming resampler."""

    def __init__(self, batch, max_push_samples, device=0):
        if not torch.cuda.is_available():
            raise PpgError('ppgs_amd: no HIP device visible; the frontend has no CPU path')
        self.device = device if isinstance(device, torch.device) else torch.device('cuda', device)
        self.batch, self.max_push_samples = int(batch), int(max_push_samples)
        self._lib = library()
        handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _check(self._lib.ppg_frontend_stream_create(
                self.device.index, self.batch, self.max_push_samples, ctypes.byref(handle)))
        self._handle = handle

    def __del__(self):
        handle, self._handle = getattr(self, '_handle', None), None
        if handle:
            self._lib.ppg_frontend_stream_destroy(handle)

    def _state(self):
        received, emitted = (ctypes.c_int64 * self.batch)(), (ctypes.c_int64 * self.batch)()
        _check(self._lib.ppg_frontend_stream_state(self._handle, received, emitted))
        return list(received), list(emitted)

    @property
    def received(self):
        """samples received so far, per item"""
        return self._state()[0]

    @property
    def emitted(self):
        """mel frames emitted so far, per item"""
        return self._state()[1]

    def reset(self, item=None):
        """Make item `item` (default: every item) ready for its next recording."""
        _check(self._lib.ppg_frontend_stream_reset(self._handle, -1 if item is None else int(item)))

    def push(self, audio, counts=None, flush=False):
        """audio (batch, n_max) or (batch, 1, n_max) fp32 on the device (None: no samples, only flushes),
        counts[b] <= n_max new samples of item b (default n_max; 0 without flush: the item sits out), flush: bool
        or one per item -> (mel fp16 (batch, 80, k_max), frames): item b's new frames are mel[b, :, :frames[b]]
        (the columns behind them are zero), k_max = max(frames)."""
        if audio is None:
            audio = torch.empty(self.batch, 0, dtype=torch.float32, device=self.device)
        if audio.dim() == 3 and audio.shape[1] == 1:
            audio = audio[:, 0]
        if audio.dim() != 2 or audio.shape[0] != self.batch:
            raise ValueError(f'audio must be ({self.batch}, samples), got {tuple(audio.shape)}')
        audio = audio.to(device=self.device, dtype=torch.float32)
        if audio.shape[1] and (audio.stride(1) != 1 or (self.batch > 1 and audio.stride(0) < audio.shape[1])):
            audio = audio.contiguous()
        nmax = audio.shape[1]
        counts = [nmax] * self.batch if counts is None else [int(n) for n in counts]
        flushes = [bool(flush)] * self.batch if isinstance(flush, bool) else [bool(f) for f in flush]
        if len(counts) != self.batch or len(flushes) != self.batch:
            raise ValueError('counts / flush need one entry per item')
        received, emitted = self._state()
        new = [audio_stream_frames(received[b] + counts[b], flushes[b]) - emitted[b] if counts[b] or flushes[b] else 0
               for b in range(self.batch)]
        kmax = max(max(new), 0)
        array = ctypes.c_int * self.batch
        frames = array()
        with torch.cuda.device(self.device):
            ragged = any(k != kmax for k in new)
            mel = (torch.zeros if ragged else torch.empty)(
                (self.batch, config.NUM_MELS, kmax), dtype=torch.float16, device=self.device)
            _check(self._lib.ppg_frontend_stream_push(
                self._handle, ctypes.c_void_p(audio.data_ptr()) if nmax else None,
                audio.stride(0) if nmax else 0, nmax, array(*counts), array(*[int(f) for f in flushes]),
                ctypes.c_void_p(mel.data_ptr()) if kmax else None, kmax, kmax, None, frames,
                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return mel, list(frames)


def _audio_engine(engine):
    if not engine.is_causal:
        raise ValueError('audio streams need a causal engine (is_causal=True), like Engine.stream')
    if engine.input_channels != config.NUM_MELS:
        raise ValueError(f'audio streams feed mel frames: the engine has {engine.input_channels} input channels, not {config.NUM_MELS}')


class AudioStream:
    """:class:`Stream` fed with raw 16 kHz samples: a :class:`FrontendStream` turns each piece into the mel
    frames it completed and the KV-cached stream emits the posteriors that became final.  Equal to Stream pushed
    with the mel of the whole recording in the same frame pieces.  Latency: 592 samples of look-ahead, up to one
    hop while a frame waits for its pair partner, and the model's 4 frames.  16 kHz only (no streaming
    resampler); causal engines with 80 input channels."""

    def __init__(self, engine, max_frames, max_push_samples=16000):
        _audio_engine(engine)
        self.engine = engine
        self.frontend = FrontendStream(1, max_push_samples, engine.device)
        self.stream = self._make_stream(engine, max_frames)

    @staticmethod
    def _make_stream(engine, max_frames):
        return Stream(engine, max_frames, torch.float16)

    def push(self, samples, flush=False, softmax=True):
        """samples (n,), (1, n) or (1, 1, n) fp32 (None or n = 0 with flush=True to just end the recording) ->
        (40, k) fp32: the posteriors of the k frames that became final."""
        engine = self.engine
        if samples is None:
            samples = torch.empty(0, dtype=torch.float32, device=engine.device)
        samples = samples.reshape(1, -1)
        step = self.frontend.max_push_samples
        pieces = []
        for start in range(0, max(samples.shape[1], 1), step):
            last = start + step >= samples.shape[1]
            mel, frames = self.frontend.push(samples[:, start:start + step], flush=flush and last)
            if frames[0] or (flush and last):
                pieces.append(self.stream.push(mel[0, :, :frames[0]], flush=flush and last, softmax=softmax))
        if not pieces:
            return torch.empty(engine.output_channels, 0, dtype=torch.float32, device=engine.device)
        return pieces[0] if len(pieces) == 1 else torch.cat(pieces, dim=1)


class LongAudioStream(AudioStream):
    """:class:`LongStream` (an utterance of more than 500 frames, as the reference chunks it) fed with raw
    16 kHz samples; see :class:`AudioStream`."""

    def __init__(self, engine, max_push_samples=16000):
        super().__init__(engine, None, max_push_samples)

    @staticmethod
    def _make_stream(engine, max_frames):
        return LongStream(engine, torch.float16)


class BatchedAudioStream:
    """:class:`BatchedStream` fed with raw 16 kHz samples: one incremental-frontend launch and one model step
    advance all `batch` recordings, each by its own number of samples; see :class:`AudioStream`."""

    def __init__(self, engine, batch, max_frames, max_push_samples=16000):
        _audio_engine(engine)
        self.engine, self.batch = engine, int(batch)
        self.frontend = FrontendStream(batch, max_push_samples, engine.device)
        self.stream = BatchedStream(engine, batch, max_frames, torch.float16)

    def push(self, samples, counts=None, flush=False, softmax=True):
        """samples (batch, n_max) fp32, n_max <= max_push_samples (None: only flushes), counts[b] new samples of
        item b, flush: bool or one per item -> a list of (40, k_b) fp32 tensors, as BatchedStream.push."""
        mel, frames = self.frontend.push(samples, counts, flush)
        return self.stream.push(mel, frames, flush, softmax)


class Stream:
    """Streaming causal inference over ONE utterance (include/ppgs_amd.h: ppg_stream_*).

    The reference has no streaming mode: its causal configuration runs every chunk as an
    independent forward (ppgs/config/causal_transformer.py:18).  A Stream produces what the
    causal forward of the whole utterance (one window, <= 500 frames) produces, a chunk at
    a time, keeping K / V^T and the residual rows of everything seen on the device.  Both
    5-tap convolutions look two frames ahead, so push() returns the posteriors that became
    final: frames < received - 4 (all of them after flush=True)."""

    def __init__(self, engine, max_frames, dtype=torch.float16):
        if dtype not in (torch.float16, torch.float32):
            raise ValueError('stream features are fp16 or fp32')
        self.engine = engine
        self.dtype = dtype
        self._lib = engine._lib
        handle = ctypes.c_void_p()
        with torch.cuda.device(engine.device):
            _check(self._lib.ppg_stream_create(
                engine._handle, int(max_frames), 0 if dtype == torch.float16 else 1,
                ctypes.byref(handle)))
        self._handle = handle
        rows = ctypes.c_int()
        _check(self._lib.ppg_stream_rows(self._handle, ctypes.byref(rows), None, None))
        self.rows = rows.value
        self.max_frames = int(max_frames)

    def __del__(self):
        handle, self._handle = getattr(self, '_handle', None), None
        if handle:
            self._lib.ppg_stream_destroy(handle)

    @property
    def received(self):
        value = ctypes.c_int()
        _check(self._lib.ppg_stream_rows(self._handle, None, ctypes.byref(value), None))
        return value.value

    def push(self, chunk, flush=False, softmax=True):
        """chunk (input_channels, n) on the engine's GPU (n may be 0 with flush=True) ->
        (40, k) fp32: the posteriors (logits if softmax=False) of the k frames that became
        final with this chunk, in order."""
        engine = self.engine
        if chunk is None:
            chunk = torch.empty(engine.input_channels, 0, dtype=self.dtype, device=engine.device)
        if chunk.dim() != 2 or chunk.shape[0] != engine.input_channels:
            raise ValueError(f'chunk must be ({engine.input_channels}, frames), got {tuple(chunk.shape)}')
        chunk = chunk.to(device=engine.device, dtype=self.dtype).contiguous()
        first, count = ctypes.c_int(), ctypes.c_int()
        with torch.cuda.device(engine.device):
            stream = torch.cuda.current_stream().cuda_stream
            _check(self._lib.ppg_stream_push(
                self._handle, ctypes.c_void_p(chunk.data_ptr()), chunk.shape[1], int(flush),
                int(softmax), ctypes.byref(first), ctypes.byref(count),
                ctypes.c_void_p(stream)))
            out = torch.empty(engine.output_channels, count.value, dtype=torch.float32,
                              device=engine.device)
            if count.value:
                # the stream owns (output_channels, rows) fp32; copy the newly final columns out
                # (ordered behind the step on the current stream)
                address = self._lib.ppg_stream_posteriors(self._handle)
                source = _device_view(address, (engine.output_channels, self.rows), engine.device)
                out.copy_(source[:, first.value:first.value + count.value])
        return out


class BatchedStream:
    """KV-cached streaming causal inference for `batch` utterances advanced together (ppg_stream_create_batch /
    ppg_stream_push_batch): configs[4] of the reference -- causal_transformer, streaming chunks, batch = 64 -- with
    the state the reference does not keep.  Item b is an utterance of its own (one window, <= 500 frames) with its
    own frontier: a push hands every item its own number of new frames (ragged, not aligned to anything, 0 = the
    item sits this step out) and ONE launch sequence advances them all.  Each item equals the causal forward of
    its whole utterance, like :class:`Stream`.

    Invariants (tests/test_gpu_stream_probe.py holds them against float64 probes in all four precisions):
    * emission: after every step item b has emitted max(received - 4, 0) frames, all of them once flushed;
    * cadence: an item's outputs do not depend on how its frames were cut into pushes -- bit for bit, in the
      default form and in the PPGS_AMD_STREAM_FUSED=2 form (the form, and the number of groups the FFN sums its
      hidden chunks in, are properties of the stream, fixed when it is created);
    * neighbours: an item's bits do not depend on what the other items of the batch are pushed, or when."""

    def __init__(self, engine, batch, max_frames, dtype=torch.float16):
        if dtype not in (torch.float16, torch.float32):
            raise ValueError('stream features are fp16 or fp32')
        self.engine, self.dtype, self.batch = engine, dtype, int(batch)
        self._lib = engine._lib
        handle = ctypes.c_void_p()
        with torch.cuda.device(engine.device):
            _check(self._lib.ppg_stream_create_batch(
                engine._handle, self.batch, int(max_frames), 0 if dtype == torch.float16 else 1,
                ctypes.byref(handle)))
        self._handle = handle
        rows = ctypes.c_int()
        _check(self._lib.ppg_stream_rows(self._handle, ctypes.byref(rows), None, None))
        self.rows = rows.value
        self.max_frames = int(max_frames)
        self.received = [0] * self.batch
        address = self._lib.ppg_stream_posteriors(self._handle)
        self._posteriors = _device_view(
            address, (self.batch, engine.output_channels, self.rows), engine.device)

    def __del__(self):
        handle, self._handle = getattr(self, '_handle', None), None
        if handle:
            self._lib.ppg_stream_destroy(handle)

    def push(self, chunks, counts=None, flush=False, softmax=True):
        """chunks (batch, input_channels, n_max) on the engine's GPU (or None with only flushes), counts[b] <= n_max
        new frames of item b (default: n_max for every item), flush: bool or one bool per item -> a list of
        (40, k_b) fp32 tensors: the posteriors of item b's frames that became final with this step, in order."""
        engine = self.engine
        if chunks is None:
            chunks = torch.empty(self.batch, engine.input_channels, 0, dtype=self.dtype, device=engine.device)
        if chunks.dim() != 3 or chunks.shape[0] != self.batch or chunks.shape[1] != engine.input_channels:
            raise ValueError(f'chunks must be ({self.batch}, {engine.input_channels}, frames), got {tuple(chunks.shape)}')
        chunks = chunks.to(device=engine.device, dtype=self.dtype).contiguous()
        nmax = chunks.shape[2]
        counts = [nmax] * self.batch if counts is None else [int(n) for n in counts]
        flushes = [bool(flush)] * self.batch if isinstance(flush, bool) else [bool(f) for f in flush]
        if len(counts) != self.batch or len(flushes) != self.batch:
            raise ValueError('counts / flush need one entry per item')
        array = ctypes.c_int * self.batch
        first, final = array(), array()
        with torch.cuda.device(engine.device):
            stream = torch.cuda.current_stream().cuda_stream
            _check(self._lib.ppg_stream_push_batch(
                self._handle, ctypes.c_void_p(chunks.data_ptr()), nmax, array(*counts),
                array(*[int(f) for f in flushes]), int(softmax), first, final, ctypes.c_void_p(stream)))
            # ONE copy (ordered behind the step on the current stream; the stream object owns the source): the column
            # range all newly final frames lie in, of every item; the results are views of it
            spans = [(first[b], first[b] + final[b]) for b in range(self.batch) if final[b] > 0]
            lo = min((a for a, _ in spans), default=0)
            hi = max((b for _, b in spans), default=0)
            block = self._posteriors[:, :, lo:hi].clone()
            out = [block[b, :, first[b] - lo:first[b] - lo + final[b]] if final[b] > 0 else block[b, :, :0]
                   for b in range(self.batch)]
        for b in range(self.batch):
            self.received[b] += counts[b]
        return out


class LongStream:
    """Streaming causal inference over ONE utterance longer than a window.

    Reference Transformer.forward (ppgs/model/transformer.py:49-64) runs sequences of more than
    500 frames as independent windows of 500 rows every 400 frames over the left-replicate-padded
    sequence (row tt of window i = frame max(400 i + tt - 50, 0)), keeps rows [50, 450) of each and
    concatenates them.  A LongStream feeds every frame to the one or two windows it belongs to --
    each a KV-cached Stream -- and emits the kept rows in frame order: the causal forward of the
    whole utterance as the reference computes it for T > 500, incrementally, with the windows'
    own look-ahead of 4 frames.  (For T <= 500 the reference uses ONE unpadded window, which is
    what Stream reproduces; the regime cannot be switched once frames have been emitted.)

    Invariants (tests/test_gpu_stream_probe.py): never more than max(received - 4, 0) frames emitted before the
    flush, all of them after it; at most two windows alive; and, as for Stream, the outputs do not depend on how
    the frames were cut into pushes, bit for bit."""

    def __init__(self, engine, dtype=torch.float16):
        self.engine, self.dtype = engine, dtype
        self.chunk, self.overlap = config.CHUNK_LENGTH, config.CHUNK_OVERLAP
        self.stride = self.chunk - 2 * self.overlap
        self.received = 0
        self._windows = {}          # index -> [Stream, rows emitted so far]
        self._done = -1             # windows <= this index have emitted all their kept rows (they finish in order)
        self._first = None

    def _window(self, index):
        if index not in self._windows:
            self._windows[index] = [Stream(self.engine, self.chunk, self.dtype), 0]
        return self._windows[index]

    def _emit(self, index, out, total=None):
        """rows of window `index` that became final -> the kept ones (as frames, in order)"""
        entry = self._windows[index]
        first = entry[1]
        entry[1] += out.shape[1]
        rows = torch.arange(first, entry[1], device=out.device)
        keep = (rows >= self.overlap) & (rows < self.chunk - self.overlap)
        if total is not None:
            keep &= (self.stride * index + rows - self.overlap) < total
        return out[:, keep]

    def push(self, chunk, flush=False, softmax=True):
        """chunk (input_channels, n) -> (40, k): the posteriors of the k frames that became final."""
        engine = self.engine
        if chunk is None:
            chunk = torch.empty(engine.input_channels, 0, dtype=self.dtype, device=engine.device)
        chunk = chunk.to(device=engine.device, dtype=self.dtype)
        n = chunk.shape[1]
        if self._first is None and n:
            self._first = chunk[:, :1]
        pieces = []
        lo, hi = self.received, self.received + n
        if n:
            first_window = max((lo + self.overlap - (self.chunk - 1) + self.stride - 1) // self.stride, 0)
            last_window = (hi - 1 + self.overlap) // self.stride
            for index in range(max(first_window, self._done + 1), last_window + 1):
                # (a finished window's last `overlap` rows keep arriving: nobody keeps them, and feeding them
                # would re-create its Stream -- workspace, K/V caches, a device synchronisation -- for nothing)
                # window rows tt = f - stride * index + overlap in [0, chunk)
                f0 = max(lo, self.stride * index - self.overlap)
                f1 = min(hi, self.stride * index - self.overlap + self.chunk)
                if f1 <= f0:
                    continue
                rows = chunk[:, f0 - lo:f1 - lo]
                if index == 0 and f0 == 0:        # the replicate padding on the left of the first window
                    rows = torch.cat([self._first.expand(-1, self.overlap), rows], dim=1)
                stream = self._window(index)[0]
                pieces.append(self._emit(index, stream.push(rows, softmax=softmax)))
        self.received = hi
        if flush:
            total = self.received
            for index in sorted(self._windows):
                stream = self._windows[index][0]
                if self.stride * index < total:   # a window whose kept rows start past the end does not exist
                    pieces.append(self._emit(index, stream.push(None, flush=True, softmax=softmax), total))
            self._windows.clear()
            self._done = (self.received + self.overlap - 1) // self.stride if self.received else -1
        else:
            # windows that have emitted all their kept rows are done
            for index in [i for i, entry in self._windows.items() if entry[1] >= self.chunk - self.overlap]:
                del self._windows[index]
                self._done = max(self._done, index)
        if not pieces:
            return torch.empty(engine.output_channels, 0, dtype=torch.float32, device=engine.device)
        return torch.cat(pieces, dim=1)


def _device_view(address, shape, device):
    """fp32 tensor view of device memory the library owns (no copy)."""
    import numpy as np

    class _Holder:
        pass
    holder = _Holder()
    count = int(np.prod(shape))
    holder.__cuda_array_interface__ = {
        'shape': (count,), 'typestr': '<f4', 'data': (int(address), False), 'version': 2}
    return torch.as_tensor(holder, device=device).view(*shape)


class W2v2FeatureEncoder:
    """The wav2vec 2.0 convolutional feature encoder on the HIP engine
    (ppg_w2v2_*): HF ``Wav2Vec2Model.feature_extractor`` -- seven strided
    convolutions, GroupNorm on the first, exact GELU -- from its state dict
    (keys ``conv_layers.{l}.conv.weight``, ``conv_layers.0.layer_norm.*``)."""

    def __init__(self, state, device=0, precision='fp16'):
        if not torch.cuda.is_available():
            raise PpgError(
                'ppgs_amd: no HIP device visible; the engine has no CPU path')
        lib = library()
        keep = []

        def ptr(key):
            tensor = state[key].detach().to('cpu', torch.float32).contiguous()
            keep.append(tensor)
            return ctypes.cast(tensor.data_ptr(), _FP)
        wts = PpgW2v2Weights()
        for layer in range(7):
            wts.conv_weight[layer] = ptr(f'conv_layers.{layer}.conv.weight')
        wts.norm_weight = ptr('conv_layers.0.layer_norm.weight')
        wts.norm_bias = ptr('conv_layers.0.layer_norm.bias')
        expected = [(512, 1, 10)] + [(512, 512, 3)] * 4 + [(512, 512, 2)] * 2
        shapes = [tuple(state[f'conv_layers.{i}.conv.weight'].shape) for i in range(7)]
        if shapes != expected:
            raise ValueError(f'not a wav2vec2-base feature encoder: conv weights {shapes}')
        handle = ctypes.c_void_p()
        _check(lib.ppg_w2v2_create(
            ctypes.byref(wts), PRECISIONS[precision], device, ctypes.byref(handle)))
        self._handle, self._lib = handle, lib
        self.device = torch.device('cuda', device)
        self.precision = precision
        self._workspaces = {}

    def __del__(self):
        handle = getattr(self, '_handle', None)
        if handle:
            self._lib.ppg_w2v2_destroy(handle)
            self._handle = None

    def frames(self, samples):
        return int(self._lib.ppg_w2v2_frames(int(samples)))

    def __call__(self, audio):
        """audio (batch, samples) fp32 on this GPU -> (batch, frames, 512) fp32
        (HF ``extract_features`` before the feature projection)."""
        if audio.dim() != 2:
            raise ValueError(f'audio must be (batch, samples), got {tuple(audio.shape)}')
        audio = audio.to(self.device, torch.float32).contiguous()
        batch, samples = audio.shape
        frames = self.frames(samples)
        if frames < 1:
            raise ValueError(f'{samples} samples are too few for the conv stack')
        size = ctypes.c_size_t()
        _check(self._lib.ppg_w2v2_workspace_bytes(self._handle, batch, samples, ctypes.byref(size)))
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
            workspace = self._workspaces.get(stream)
            if workspace is None or workspace.numel() < size.value:
                workspace = torch.empty(size.value, dtype=torch.uint8, device=self.device)
                self._workspaces[stream] = workspace
            out = torch.empty((batch, frames, 512), dtype=torch.float32, device=self.device)
            _check(self._lib.ppg_w2v2_features(
                self._handle, audio.data_ptr(), batch, samples, out.data_ptr(),
                workspace.data_ptr(), workspace.numel(), stream))
        return out


def _weight_normed(conv, dim=2):
    """The effective weight of a weight-normalised convolution (HF's positional convolution:
    weight_norm(name='weight', dim=2)), computed from g and v -- with the legacy
    torch.nn.utils.weight_norm `.weight` is a plain attribute that only the forward pre-hook
    refreshes, so after from_pretrained it can be stale."""
    parametrizations = getattr(conv, 'parametrizations', None)
    if parametrizations is not None and 'weight' in parametrizations:
        g, v = parametrizations.weight.original0, parametrizations.weight.original1
    elif hasattr(conv, 'weight_g') and hasattr(conv, 'weight_v'):
        g, v = conv.weight_g, conv.weight_v
    else:
        return conv.weight
    return torch._weight_norm(v.detach().float(), g.detach().float(), dim)


class W2v2Body:
    """The wav2vec 2.0 transformer body on the HIP engine (ppg_w2v2_body_*): HF
    ``Wav2Vec2Model``'s ``feature_projection`` + ``encoder`` (post-norm layers, grouped
    positional convolution), built from the HF module's parameters."""

    def __init__(self, model, device=0, precision='fp16'):
        if not torch.cuda.is_available():
            raise PpgError('ppgs_amd: no HIP device visible; the engine has no CPU path')
        lib = library()
        cfg = model.config
        if getattr(cfg, 'do_stable_layer_norm', False):
            raise ValueError('the HIP wav2vec2 body implements the post-norm encoder (do_stable_layer_norm = False)')
        keep = []

        def ptr(tensor):
            tensor = tensor.detach().to('cpu', torch.float32).contiguous()
            keep.append(tensor)
            return ctypes.cast(tensor.data_ptr(), _FP)
        wts = PpgW2v2BodyWeights()
        wts.hidden, wts.heads, wts.ffn = cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size
        wts.num_layers = len(model.encoder.layers)
        wts.conv_kernel, wts.conv_groups = cfg.num_conv_pos_embeddings, cfg.num_conv_pos_embedding_groups
        wts.layer_norm_eps = cfg.layer_norm_eps
        projection, encoder = model.feature_projection, model.encoder
        wts.proj_norm_weight, wts.proj_norm_bias = ptr(projection.layer_norm.weight), ptr(projection.layer_norm.bias)
        wts.proj_weight, wts.proj_bias = ptr(projection.projection.weight), ptr(projection.projection.bias)
        conv = encoder.pos_conv_embed.conv
        wts.pos_conv_weight, wts.pos_conv_bias = ptr(_weight_normed(conv)), ptr(conv.bias)
        wts.enc_norm_weight, wts.enc_norm_bias = ptr(encoder.layer_norm.weight), ptr(encoder.layer_norm.bias)
        for index, layer in enumerate(encoder.layers):
            lw, attn = wts.layers[index], layer.attention
            lw.q_weight, lw.q_bias = ptr(attn.q_proj.weight), ptr(attn.q_proj.bias)
            lw.k_weight, lw.k_bias = ptr(attn.k_proj.weight), ptr(attn.k_proj.bias)
            lw.v_weight, lw.v_bias = ptr(attn.v_proj.weight), ptr(attn.v_proj.bias)
            lw.out_weight, lw.out_bias = ptr(attn.out_proj.weight), ptr(attn.out_proj.bias)
            lw.norm1_weight, lw.norm1_bias = ptr(layer.layer_norm.weight), ptr(layer.layer_norm.bias)
            lw.ffn1_weight = ptr(layer.feed_forward.intermediate_dense.weight)
            lw.ffn1_bias = ptr(layer.feed_forward.intermediate_dense.bias)
            lw.ffn2_weight = ptr(layer.feed_forward.output_dense.weight)
            lw.ffn2_bias = ptr(layer.feed_forward.output_dense.bias)
            lw.norm2_weight, lw.norm2_bias = ptr(layer.final_layer_norm.weight), ptr(layer.final_layer_norm.bias)
        handle = ctypes.c_void_p()
        _check(lib.ppg_w2v2_body_create(
            ctypes.byref(wts), PRECISIONS[precision], device, ctypes.byref(handle)))
        self._handle, self._lib = handle, lib
        self.device = torch.device('cuda', device)
        self.precision = precision
        self.hidden = cfg.hidden_size
        self._workspaces = {}

    def __del__(self):
        handle = getattr(self, '_handle', None)
        if handle:
            self._lib.ppg_w2v2_body_destroy(handle)
            self._handle = None

    def __call__(self, features, valid_frames):
        """features (batch, frames, 512) fp32 on this GPU (HF ``extract_features``), valid frames
        per item (HF's frame-level attention mask as lengths) -> ``last_hidden_state``
        (batch, frames, hidden) fp32."""
        if features.dim() != 3 or features.shape[2] != 512:
            raise ValueError(f'features must be (batch, frames, 512), got {tuple(features.shape)}')
        features = features.to(self.device, torch.float32).contiguous()
        batch, frames, _ = features.shape
        arr = _lengths_array(valid_frames, batch)
        size = ctypes.c_size_t()
        _check(self._lib.ppg_w2v2_body_workspace_bytes(self._handle, batch, frames, ctypes.byref(size)))
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
            workspace = self._workspaces.get(stream)
            if workspace is None or workspace.numel() < size.value:
                workspace = torch.empty(size.value, dtype=torch.uint8, device=self.device)
                self._workspaces[stream] = workspace
            out = torch.empty((batch, frames, self.hidden), dtype=torch.float32, device=self.device)
            _check(self._lib.ppg_w2v2_body_forward(
                self._handle, features.data_ptr(), arr, batch, frames, out.data_ptr(),
                workspace.data_ptr(), workspace.numel(), stream))
        return out


def frontend_profile(device, enable=True):
    _check(library().ppg_frontend_profile(device, int(enable)))


def frontend_profile_read(device):
    total, count = ctypes.c_double(), ctypes.c_int64()
    _check(library().ppg_frontend_profile_read(
        device, ctypes.byref(total), ctypes.byref(count)))
    return total.value, count.value


###############################################################################
# Native file ingest / output (host only)
###############################################################################


def _paths_array(paths):
    encoded = [os.fsencode(os.fspath(p)) for p in paths]
    return (ctypes.c_char_p * len(encoded))(*encoded)


def _check_io(code):
    if code < 0:
        raise ValueError('ppgs_amd: ' + library().ppg_io_last_error().decode())


def wav_info(path):
    """(samples per channel, sample rate, channels) from the RIFF header."""
    samples, rate, channels = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
    _check_io(library().ppg_wav_info(
        os.fsencode(os.fspath(path)), ctypes.byref(samples), ctypes.byref(rate),
        ctypes.byref(channels)))
    return samples.value, rate.value, channels.value


def wav_read_batch(paths, max_samples, threads=4, pin_memory=None):
    """Decode WAV files into one zero-padded (B, 1, max_samples) fp32 tensor
    (pinned when a GPU is present) -> (tensor, samples (B,), rates list)."""
    count = len(paths)
    if pin_memory is None:
        pin_memory = torch.cuda.is_available()
    batch = torch.empty((count, 1, max_samples), dtype=torch.float32,
                        pin_memory=pin_memory)
    samples = (ctypes.c_int64 * count)()
    rates = (ctypes.c_int32 * count)()
    _check_io(library().ppg_wav_read_batch(
        _paths_array(paths), count, batch.data_ptr(), max_samples, max_samples,
        samples, rates, int(threads)))
    return batch, torch.tensor(list(samples), dtype=torch.long), list(rates)


def pt_write_batch(paths, tensor, lengths, threads=4):
    """Write tensor[i, :, :lengths[i]] (fp32, CPU, (B, rows, T) contiguous) as
    torch.load-able .pt files."""
    if tensor.is_cuda or tensor.dtype != torch.float32 or tensor.dim() != 3:
        raise ValueError('pt_write_batch expects a CPU fp32 (B, rows, T) tensor')
    tensor = tensor.contiguous()
    count, rows, frames = tensor.shape
    cols = (ctypes.c_int64 * count)(*[int(v) for v in lengths])
    _check_io(library().ppg_pt_write_batch(
        _paths_array(paths), count, tensor.data_ptr(), rows * frames, rows,
        frames, cols, int(threads)))
