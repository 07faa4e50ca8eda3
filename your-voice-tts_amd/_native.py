"""ctypes binding of libtts_hip.so (C-ABI in include/tts_hip.h).

The library is loaded on first use.  If it is missing, fails to load, or no GPU is visible, the
caller gets a RuntimeError: the product path has no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TTS_HIP_LIB", os.path.join(_HERE, "libtts_hip.so"))

TTS_GL_FROM_MEL = 0
TTS_GL_FROM_LINEAR = 1
TTS_LOSS_L1 = 0
TTS_LOSS_MSE = 1
TTS_LOSS_BCE = 2  # tts_loss_backward only
TTS_OPTIM_CHUNK = 8192  # elements per chunk of work of csrc/optim.hip (include/tts_hip.h)
GL_PATHS = {0: "unfused", 1: "fused", 2: "persistent"}  # TTS_GL_PATH_* (include/tts_hip.h)
DECODER_STEP_KERNELS = ("prenet2", "att_lstm", "query", "attention", "dec_lstm", "mel_fused")
GL_KERNELS = ("gl_iter", "gl_ola")
TACOTRON_STEP_KERNELS = ("prenet2", "att_gru", "query", "attention", "proj", "dec_gru1", "dec_gru2", "mel",
                         "pre1_stop")

# every symbol include/tts_hip.h declares
EXPORTS = (
    "tts_encoder_create", "tts_encoder_destroy", "tts_encoder_run", "tts_encoder_run_state", "tts_encoder_last_path",
    "tts_encoder_add_speakers", "tts_synth_run_speakers",
    "tts_encoder_counters", "tts_encoder_status_rule", "tts_synth_state",
    "tts_decoder_create", "tts_decoder_destroy", "tts_decoder_run", "tts_decoder_run_continue", "tts_decoder_run_teacher",
    "tts_decoder_last_timing", "tts_decoder_last_path", "tts_decoder_resident_limits", "tts_decoder_resident_phases", "tts_decoder_resident_trace",
    "tts_decoder_profile",
    "tts_postnet_create", "tts_postnet_destroy", "tts_postnet_run", "tts_postnet_last_path",
    "tts_gl_create", "tts_gl_destroy", "tts_gl_run", "tts_gl_last_timing", "tts_gl_last_path", "tts_gl_profile",
    "tts_gl_set_mel_basis", "tts_gl_melspectrogram", "tts_gl_set_phase_state", "tts_gl_get_phase_state",
    "tts_gl_draw_phases", "tts_gl_save_pcm16", "tts_gl_analyze", "tts_gl_linear_to_mel",
    "tts_gl_trim_silence", "tts_gl_find_endpoint", "tts_gl_take_segments",
    "tts_gl_set_resample_filter", "tts_gl_resample",
    "tts_synth_create", "tts_synth_destroy", "tts_synth_run", "tts_synth_sync",
    "tts_tacotron_create", "tts_tacotron_destroy", "tts_tacotron_encode", "tts_tacotron_encode_last_path",
    "tts_tacotron_decode",
    "tts_tacotron_decode_teacher",
    "tts_tacotron_postnet", "tts_tacotron_last_timing", "tts_tacotron_last_path", "tts_tacotron_resident_phases",
    "tts_tacotron_profile",
    "tts_loss_create", "tts_loss_destroy", "tts_loss_masked", "tts_loss_bce_logits", "tts_loss_backward",
    "tts_optim_create", "tts_optim_destroy", "tts_optim_set_tensors", "tts_optim_grad_norm", "tts_optim_clip",
    "tts_optim_decay", "tts_optim_adam", "tts_optim_step",
    "tts_lstm_create", "tts_lstm_destroy", "tts_lstm_set_weights", "tts_lstm_reserve_floats", "tts_lstm_forward",
    "tts_lstm_backward",
    "tts_gru_create", "tts_gru_destroy", "tts_gru_set_weights", "tts_gru_reserve_floats", "tts_gru_forward",
    "tts_gru_backward",
    "tts_convbn_create", "tts_convbn_destroy", "tts_convbn_set_weights", "tts_convbn_reserve_floats",
    "tts_convbn_forward", "tts_convbn_backward",
    "tts_dectrain_create", "tts_dectrain_destroy", "tts_dectrain_set_weights", "tts_dectrain_reserve_floats",
    "tts_dectrain_forward", "tts_dectrain_backward",
    "tts_last_error", "tts_version",
)


class TensorView(ctypes.Structure):
    _fields_ = [("key", ctypes.c_char_p), ("data", ctypes.c_void_p), ("numel", ctypes.c_int64)]


class DecoderConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        "r", "attn_norm", "forward_attn", "trans_agent", "forward_attn_mask", "location_attn",
        "windowing", "max_batch", "max_len", "max_steps")]


class TacotronConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        "r", "memory_size", "attn_norm", "forward_attn", "trans_agent", "forward_attn_mask", "location_attn",
        "windowing", "gst", "num_speakers", "max_batch", "max_len", "max_steps")]


class OptimTensor(ctypes.Structure):  # tts_optim_tensor
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("numel", ctypes.c_int64), ("step", ctypes.c_int64)]


class AudioConfig(ctypes.Structure):
    _fields_ = [("n_fft", ctypes.c_int), ("hop_length", ctypes.c_int), ("win_length", ctypes.c_int),
                ("num_mels", ctypes.c_int), ("min_level_db", ctypes.c_float),
                ("ref_level_db", ctypes.c_float), ("power", ctypes.c_float),
                ("max_norm", ctypes.c_float), ("preemphasis", ctypes.c_double),
                ("signal_norm", ctypes.c_int), ("symmetric_norm", ctypes.c_int), ("clip_norm", ctypes.c_int)]


# tts_dectrain_weights / tts_dectrain_grads: the reference Decoder's parameters, state-dict name -> field order
DECTRAIN_PARAMS = (
    "prenet.layers.0.linear_layer.weight", "prenet.layers.1.linear_layer.weight",
    "attention_rnn.weight_ih", "attention_rnn.weight_hh", "attention_rnn.bias_ih", "attention_rnn.bias_hh",
    "attention_layer.query_layer.linear_layer.weight", "attention_layer.inputs_layer.linear_layer.weight",
    "attention_layer.v.linear_layer.weight", "attention_layer.v.linear_layer.bias",
    "decoder_rnn.weight_ih", "decoder_rnn.weight_hh", "decoder_rnn.bias_ih", "decoder_rnn.bias_hh",
    "linear_projection.linear_layer.weight", "linear_projection.linear_layer.bias",
    "stopnet.1.linear_layer.weight", "stopnet.1.linear_layer.bias",
    "attention_rnn_init.weight", "go_frame_init.weight", "decoder_rnn_inits.weight")
DECTRAIN_MASKS = ("prenet1", "prenet2", "att_h", "att_c", "dec_h", "dec_c", "stop")


class DectrainTensors(ctypes.Structure):  # tts_dectrain_weights, tts_dectrain_grads
    _fields_ = [(f"p{i}", ctypes.c_void_p) for i in range(len(DECTRAIN_PARAMS))]


class DectrainMasks(ctypes.Structure):  # tts_dectrain_masks
    _fields_ = [(n, ctypes.c_void_p) for n in DECTRAIN_MASKS] + [
        ("scale_prenet", ctypes.c_float), ("scale_rnn", ctypes.c_float), ("scale_stop", ctypes.c_float)]


_lib = None
_lock = threading.Lock()
P = ctypes.c_void_p
I32P = ctypes.POINTER(ctypes.c_int32)


def _declare(lib):
    vp = ctypes.c_void_p
    lib.tts_encoder_create.argtypes = [ctypes.POINTER(TensorView), ctypes.c_int, ctypes.c_int, ctypes.c_int, vp,
                                       ctypes.POINTER(vp)]
    lib.tts_encoder_destroy.argtypes = [vp]
    lib.tts_encoder_destroy.restype = None
    lib.tts_encoder_run.argtypes = [vp, vp, I32P, ctypes.c_int, ctypes.c_int, vp, vp]
    lib.tts_encoder_add_speakers.argtypes = [vp, vp, I32P, I32P, ctypes.c_int, ctypes.c_int, vp]
    lib.tts_decoder_create.argtypes = [ctypes.POINTER(DecoderConfig), ctypes.POINTER(TensorView), ctypes.c_int, vp,
                                       ctypes.POINTER(vp)]
    lib.tts_decoder_destroy.argtypes = [vp]
    lib.tts_decoder_destroy.restype = None
    lib.tts_decoder_run.argtypes = [vp, vp, I32P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp,
                                    I32P, vp]
    lib.tts_encoder_run_state.argtypes = [vp, vp, I32P, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
    lib.tts_decoder_run_continue.argtypes = lib.tts_decoder_run.argtypes
    lib.tts_decoder_run_teacher.argtypes = [vp, vp, I32P, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int64, ctypes.c_int,
                                            vp, vp, vp, vp]
    lib.tts_decoder_last_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)]
    lib.tts_decoder_last_path.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    lib.tts_decoder_resident_limits.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.tts_encoder_last_path.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    lib.tts_gl_last_path.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    lib.tts_synth_sync.argtypes = [vp]
    IP = ctypes.POINTER(ctypes.c_int)
    lib.tts_encoder_counters.argtypes = [vp, IP, IP]
    lib.tts_encoder_status_rule.argtypes = [ctypes.c_int, ctypes.c_uint, IP, IP, IP]
    lib.tts_synth_state.argtypes = [vp, IP, IP]
    lib.tts_decoder_resident_phases.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.c_int]
    lib.tts_decoder_resident_trace.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong), ctypes.c_int64]
    lib.tts_postnet_create.argtypes = [ctypes.POINTER(TensorView), ctypes.c_int, ctypes.c_int, vp, ctypes.POINTER(vp)]
    lib.tts_postnet_destroy.argtypes = [vp]
    lib.tts_postnet_destroy.restype = None
    lib.tts_postnet_run.argtypes = [vp, vp, I32P, ctypes.c_int, ctypes.c_int, vp, vp]
    lib.tts_postnet_last_path.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    lib.tts_gl_create.argtypes = [ctypes.POINTER(AudioConfig), vp, vp, ctypes.POINTER(vp)]
    lib.tts_gl_destroy.argtypes = [vp]
    lib.tts_gl_destroy.restype = None
    lib.tts_gl_run.argtypes = [vp, ctypes.c_int, vp, I32P, ctypes.c_int, ctypes.c_int, vp, ctypes.c_uint64,
                               ctypes.c_int, vp, vp]
    lib.tts_gl_set_mel_basis.argtypes = [vp, vp]
    lib.tts_gl_melspectrogram.argtypes = [vp, vp, I32P, ctypes.c_int, ctypes.c_int64, vp, ctypes.c_int, vp]
    lib.tts_gl_analyze.argtypes = [vp, vp, I32P, ctypes.c_int, ctypes.c_int64, vp, vp, ctypes.c_int, vp]
    lib.tts_gl_linear_to_mel.argtypes = [vp, vp, I32P, ctypes.c_int, ctypes.c_int, vp, vp]
    lib.tts_gl_last_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)]
    U32P = ctypes.POINTER(ctypes.c_uint32)
    lib.tts_gl_set_phase_state.argtypes = [vp, U32P, ctypes.c_int]
    lib.tts_gl_get_phase_state.argtypes = [vp, U32P, ctypes.POINTER(ctypes.c_int)]
    lib.tts_gl_draw_phases.argtypes = [vp, I32P, ctypes.c_int, ctypes.c_int, vp, vp]
    lib.tts_gl_save_pcm16.argtypes = [vp, vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.c_int,
                                      ctypes.c_double, vp, vp]
    lib.tts_gl_trim_silence.argtypes = [vp, vp, ctypes.c_int64, I32P, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_double, I32P, I32P, vp]
    lib.tts_gl_find_endpoint.argtypes = [vp, vp, ctypes.c_int64, I32P, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_double, I32P, vp]
    lib.tts_gl_take_segments.argtypes = [vp, vp, ctypes.c_int64, I32P, I32P, ctypes.c_int, vp, ctypes.c_int64, vp]
    lib.tts_gl_set_resample_filter.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int]
    lib.tts_gl_resample.argtypes = [vp, vp, ctypes.c_int64, I32P, I32P, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int64,
                                    I32P, vp]
    lib.tts_synth_create.argtypes = [vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
    lib.tts_synth_destroy.argtypes = [vp]
    lib.tts_synth_destroy.restype = None
    lib.tts_synth_run.argtypes = [vp, I32P, I32P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_uint64, vp, ctypes.c_int64, I32P, vp]
    lib.tts_synth_run_speakers.argtypes = [vp, I32P, I32P, I32P, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_uint64, vp, ctypes.c_int64, I32P, vp]
    FP = ctypes.POINTER(ctypes.c_float)
    lib.tts_decoder_profile.argtypes = [vp, ctypes.c_int, FP, ctypes.c_int]
    lib.tts_gl_profile.argtypes = [vp, ctypes.c_int, FP, ctypes.c_int]
    lib.tts_tacotron_create.argtypes = [ctypes.POINTER(TacotronConfig), ctypes.POINTER(TensorView), ctypes.c_int, vp,
                                        ctypes.POINTER(vp)]
    lib.tts_tacotron_destroy.argtypes = [vp]
    lib.tts_tacotron_destroy.restype = None
    lib.tts_tacotron_encode.argtypes = [vp, vp, I32P, ctypes.c_int, ctypes.c_int, I32P, vp, ctypes.c_int, vp, vp]
    lib.tts_tacotron_encode_last_path.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    lib.tts_tacotron_decode.argtypes = [vp, vp, I32P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp,
                                        vp, I32P, vp]
    lib.tts_tacotron_decode_teacher.argtypes = [vp, vp, I32P, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int64,
                                                ctypes.c_int, vp, vp, vp, vp]
    lib.tts_tacotron_postnet.argtypes = [vp, vp, I32P, ctypes.c_int, ctypes.c_int, vp, vp]
    lib.tts_tacotron_last_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)]
    lib.tts_tacotron_last_path.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    lib.tts_tacotron_resident_phases.argtypes = [vp, FP, ctypes.c_int]
    lib.tts_tacotron_profile.argtypes = [vp, ctypes.c_int, FP, ctypes.c_int]
    DP, I64P = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    lib.tts_loss_create.argtypes = [ctypes.POINTER(vp)]
    lib.tts_loss_destroy.argtypes = [vp]
    lib.tts_loss_destroy.restype = None
    lib.tts_loss_masked.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int64, vp, ctypes.c_int64, I32P, ctypes.c_int,
                                    ctypes.c_int, ctypes.c_int, vp, vp, DP, I64P, DP, vp]
    lib.tts_loss_bce_logits.argtypes = [vp, vp, vp, ctypes.c_int64, vp, vp, DP, DP, vp]
    lib.tts_loss_backward.argtypes = [ctypes.c_int, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, ctypes.c_int,
                                      ctypes.c_int64, ctypes.c_int64, vp, vp, ctypes.c_int64, vp]
    OT, D = ctypes.POINTER(OptimTensor), ctypes.c_double
    lib.tts_optim_create.argtypes = [ctypes.POINTER(vp)]
    lib.tts_optim_destroy.argtypes = [vp]
    lib.tts_optim_destroy.restype = None
    lib.tts_optim_set_tensors.argtypes = [vp, I64P, ctypes.c_int, vp]
    lib.tts_optim_grad_norm.argtypes = [vp, OT, ctypes.c_int, D, vp, vp, DP, DP, vp]
    lib.tts_optim_clip.argtypes = lib.tts_optim_grad_norm.argtypes
    lib.tts_optim_decay.argtypes = [vp, OT, ctypes.c_int, D, D, vp]
    lib.tts_optim_adam.argtypes = [vp, OT, ctypes.c_int, D, D, D, D, vp]
    lib.tts_optim_step.argtypes = [vp, OT, ctypes.c_int, D, D, D, D, D, D, vp, vp, vp]
    PP = ctypes.POINTER(vp)
    lib.tts_lstm_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
    lib.tts_lstm_destroy.argtypes = [vp]
    lib.tts_lstm_destroy.restype = None
    lib.tts_lstm_set_weights.argtypes = [vp, PP, PP, PP, PP, vp]
    lib.tts_lstm_reserve_floats.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    lib.tts_lstm_reserve_floats.restype = ctypes.c_int64
    lib.tts_lstm_forward.argtypes = [vp, vp, I32P, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp]
    lib.tts_lstm_backward.argtypes = [vp, vp, I32P, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, PP, PP, PP, PP, vp]
    lib.tts_gru_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
    lib.tts_gru_destroy.argtypes = [vp]
    lib.tts_gru_destroy.restype = None
    lib.tts_gru_set_weights.argtypes = [vp, PP, PP, PP, PP, vp]
    lib.tts_gru_reserve_floats.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    lib.tts_gru_reserve_floats.restype = ctypes.c_int64
    lib.tts_gru_forward.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp]
    lib.tts_gru_backward.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, vp, PP, PP, PP, PP, vp]
    lib.tts_convbn_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
    lib.tts_convbn_destroy.argtypes = [vp]
    lib.tts_convbn_destroy.restype = None
    lib.tts_convbn_set_weights.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.tts_convbn_reserve_floats.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    lib.tts_convbn_reserve_floats.restype = ctypes.c_int64
    lib.tts_convbn_forward.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_float, vp, vp, D, D,
                                       ctypes.c_int, vp, vp, vp]
    lib.tts_convbn_backward.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    ci = ctypes.c_int
    lib.tts_dectrain_create.argtypes = [ci] * 9 + [ctypes.POINTER(vp)]
    lib.tts_dectrain_destroy.argtypes = [vp]
    lib.tts_dectrain_destroy.restype = None
    lib.tts_dectrain_set_weights.argtypes = [vp, ctypes.POINTER(DectrainTensors), vp]
    lib.tts_dectrain_reserve_floats.argtypes = [vp, ci, ci, ci]
    lib.tts_dectrain_reserve_floats.restype = ctypes.c_int64
    lib.tts_dectrain_forward.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ctypes.POINTER(DectrainMasks), vp, vp, vp, vp,
                                         vp]
    lib.tts_dectrain_backward.argtypes = [vp, vp, ci, ci, ci, ctypes.POINTER(DectrainMasks), vp, vp, vp, vp, vp,
                                          ctypes.POINTER(DectrainTensors), vp]
    lib.tts_last_error.restype = ctypes.c_char_p
    lib.tts_version.restype = ctypes.c_char_p
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name.endswith(("_create", "_run", "_timing", "_profile", "_encode", "_decode", "_postnet", "_state",
                          "_continue", "_basis", "_melspectrogram", "_path", "_sync", "_phases", "_teacher",
                          "_phase_state", "_pcm16", "_limits", "_analyze", "_to_mel", "_silence", "_endpoint",
                          "_segments", "_masked", "_logits", "_filter", "_resample", "_tensors", "_grad_norm",
                          "_clip", "_decay", "_adam", "_step", "_backward", "_counters", "_rule", "_weights",
                          "_forward")):
            fn.restype = ctypes.c_int


def load_library(path: str = LIB_PATH):
    """Load (once) and return the ctypes handle.  torch is imported first so that the HIP
    runtime torch ships (SONAME libamdhip64.so.7) is the one the library binds to."""
    global _lib
    with _lock:
        if _lib is None:
            import torch  # noqa: F401  (HIP runtime first)
            if not os.path.exists(path):
                raise RuntimeError(f"libtts_hip.so not found at {path}: build it with "
                                   f"`make -C your-voice-tts_amd/csrc` (no CPU fallback exists)")
            lib = ctypes.CDLL(path)
            _declare(lib)
            _lib = lib
    return _lib


def lib():
    """Library handle for compute calls: requires a visible GPU."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: the MI355X synthesis path has no CPU fallback")
    return load_library()


def check(status: int, what: str):
    if status != 0:
        msg = load_library().tts_last_error().decode(errors="replace")
        if "attention norm" in msg:
            raise RuntimeError("Unknown value for attention norm type")
        raise RuntimeError(f"{what} failed (status {status}): {msg}")


def stream_handle(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def tensor_views(tensors: dict):
    """Build a TensorView array over CUDA tensors; returns (array, keepalive)."""
    items = list(tensors.items())
    arr = (TensorView * len(items))()
    keep = []
    for i, (k, t) in enumerate(items):
        kb = k.encode()
        keep.append(kb)
        keep.append(t)
        arr[i].key = kb
        arr[i].data = t.data_ptr()
        arr[i].numel = t.numel()
    return arr, keep


def i32_array(values):
    vals = [int(v) for v in values]
    return (ctypes.c_int32 * len(vals))(*vals)
