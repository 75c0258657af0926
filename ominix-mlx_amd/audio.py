"""Host mirror of funasr-mlx's `MelFrontend` (funasr-mlx/src/paraformer.rs:195-412) over the
omx_mel_frontend_* C ABI: same constructor inputs (ParaformerConfig frontend fields), `set_cmvn`,
`forward(audio) -> [1, T', 560]`, same error for non-finite audio."""
from __future__ import annotations

import ctypes
import sys

import numpy as np

from . import OmxError, check, lib, require_device
from .ops import Tensor

c_int, c_void_p, c_int64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64


class MelConfig(ctypes.Structure):
    _fields_ = [("sample_rate", c_int), ("n_mels", c_int), ("n_fft", c_int), ("hop_length", c_int),
                ("lfr_m", c_int), ("lfr_n", c_int)]


class AudioEncoderConfig(ctypes.Structure):
    """AudioEncoderConfig (qwen3-asr-mlx/src/encoder.rs:14-72), the fields the tower's arithmetic reads"""
    _fields_ = [("n_mels", c_int), ("n_layers", c_int), ("n_heads", c_int), ("ffn_dim", c_int), ("d_model", c_int),
                ("max_source_positions", c_int), ("n_window", c_int), ("output_dim", c_int), ("n_window_infer", c_int),
                ("downsample_hidden_size", c_int)]


class FunASRNanoEncoderConfig(ctypes.Structure):
    """SenseVoiceEncoderConfig (funasr-nano-mlx/src/sensevoice_encoder.rs:20-70) and AdaptorConfig (adaptor.rs:12-53)"""
    _fields_ = [("lfr_dim", c_int), ("output_size", c_int), ("attention_heads", c_int), ("linear_units", c_int), ("num_blocks", c_int),
                ("tp_blocks", c_int), ("kernel_size", c_int), ("encoder_dim", c_int), ("ffn_dim", c_int), ("llm_dim", c_int), ("n_layer", c_int)]


class ViTConfig(ctypes.Structure):
    """ViTConfig (moxin-vlm-mlx/src/vision.rs:26-37) plus the tower's image statistics (lib.rs:427-440) and the checkpoint prefix the
    error texts name.  It lives here, beside the audio tower's, because its entry points are bound in AUDIO_SIGNATURES (vision.py uses them)."""
    _fields_ = [("embed_dim", c_int), ("depth", c_int), ("num_heads", c_int), ("head_dim", c_int), ("intermediate_dim", c_int),
                ("has_cls_token", c_int), ("num_registers", c_int), ("has_layer_scale", c_int), ("patch_size", c_int), ("image_size", c_int),
                ("mean", ctypes.c_float * 3), ("std", ctypes.c_float * 3), ("key_prefix", ctypes.c_char * 128)]


class SamConfig(ctypes.Structure):
    """The SAM ViT-B tower of DeepSeek-OCR-2 (deepseek-ocr2-mlx/src/vision.rs:492-496; omx_sam_config of include/omx.h)"""
    _fields_ = [("embed_dim", c_int), ("depth", c_int), ("num_heads", c_int), ("mlp_dim", c_int), ("window", c_int), ("patch_size", c_int),
                ("n_global", c_int), ("keep_stages", c_int), ("global_attn_indexes", c_int * 16), ("key_prefix", ctypes.c_char * 128)]


class VcfConfig(ctypes.Structure):
    """The visual-causal-flow encoder of DeepSeek-OCR-2 (qwen2_encoder.rs:305-311; omx_vcf_config of include/omx.h)"""
    _fields_ = [("hidden", c_int), ("layers", c_int), ("heads", c_int), ("kv_heads", c_int), ("intermediate", c_int), ("keep_stages", c_int),
                ("rope_theta", ctypes.c_float), ("eps", ctypes.c_float), ("key_prefix", ctypes.c_char * 128)]


AUDIO_SIGNATURES = {
    "omx_mel_frontend_create": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(MelConfig)]),
    "omx_mel_frontend_destroy": (c_int, [c_void_p]),
    "omx_mel_frontend_set_cmvn": (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    "omx_mel_frontend_frames": (c_int, [c_void_p, c_int64, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "omx_mel_frontend_forward": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "omx_whisper_mel_create": (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int]),
    "omx_whisper_mel_frames": (c_int, [c_void_p, c_int64, ctypes.POINTER(c_int)]),
    "omx_whisper_mel_forward": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "omx_sensevoice_mel_create": (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int, ctypes.c_float]),
    "omx_sensevoice_mel_frames": (c_int, [c_void_p, c_int64, ctypes.POINTER(c_int)]),
    "omx_sensevoice_mel_forward": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "omx_apply_lfr": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "omx_resample_len": (c_int64, [c_int64, ctypes.c_uint32, ctypes.c_uint32]),
    "omx_resample_sinc": (c_int, [c_void_p, c_int64, ctypes.c_uint32, ctypes.c_uint32, c_void_p, c_int64, ctypes.POINTER(c_int64), c_void_p]),
    # the Qwen3-ASR audio tower in float32 (csrc/audio_encoder.hip)
    "omx_qwen3_asr_encoder_create": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(AudioEncoderConfig)]),
    "omx_qwen3_asr_encoder_load": (c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.POINTER(c_int64), c_int]),
    "omx_qwen3_asr_encoder_tokens": (c_int, [c_void_p, c_int, ctypes.POINTER(c_int)]),
    "omx_qwen3_asr_encoder_forward": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "omx_qwen3_asr_encoder_destroy": (c_int, [c_void_p]),
    "omx_qwen3_asr_encoder_debug_read": (c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.c_size_t]),
    "omx_window_attention_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    # the Fun-ASR-Nano audio tower over stacked utterances in float32 (csrc/sensevoice_encoder.hip)
    "omx_funasr_nano_encoder_create": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(FunASRNanoEncoderConfig)]),
    "omx_funasr_nano_encoder_load": (c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.POINTER(c_int64), c_int]),
    "omx_funasr_nano_encoder_forward": (c_int, [c_void_p, c_void_p, ctypes.POINTER(c_int), c_int, c_void_p, c_void_p]),
    "omx_funasr_nano_encoder_destroy": (c_int, [c_void_p]),
    "omx_funasr_nano_encoder_debug_read": (c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.c_size_t]),
    "omx_segment_attention_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, ctypes.POINTER(c_int), c_int, c_int,
                                          c_void_p]),
    # the Moxin-VLM vision towers and projector in float32 (csrc/vit_encoder.hip; the classes are in vision.py)
    "omx_vit_encoder_create": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(ViTConfig)]),
    "omx_vit_encoder_load": (c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.POINTER(c_int64), c_int]),
    "omx_vit_encoder_tokens": (c_int, [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "omx_vit_encoder_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "omx_vit_encoder_launches": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "omx_vit_encoder_debug_read": (c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.c_size_t]),
    "omx_vit_encoder_destroy": (c_int, [c_void_p]),
    "omx_vit_attention_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    "omx_gemm_f32_epilogue": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "omx_vlm_projector_create": (c_int, [ctypes.POINTER(c_void_p)]),
    "omx_vlm_projector_load": (c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.POINTER(c_int64), c_int]),
    "omx_vlm_projector_dims": (c_int, [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "omx_vlm_projector_forward": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "omx_vlm_projector_destroy": (c_int, [c_void_p]),
    # the DeepSeek-OCR-2 vision side in float32 (csrc/sam_encoder.hip, csrc/vcf_encoder.hip; the classes are in vision.py)
    "omx_sam_attention_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
                                      c_void_p, c_void_p]),
    "omx_prefix_causal_attention_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "omx_sam_encoder_create": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(SamConfig)]),
    "omx_sam_encoder_load": (c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.POINTER(c_int64), c_int]),
    "omx_sam_encoder_tokens": (c_int, [c_void_p, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "omx_sam_encoder_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "omx_sam_encoder_launches": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "omx_sam_encoder_scratch_bytes": (c_int, [c_void_p, ctypes.POINTER(ctypes.c_size_t)]),
    "omx_sam_encoder_debug_read": (c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.c_size_t]),
    "omx_sam_encoder_destroy": (c_int, [c_void_p]),
    "omx_vcf_encoder_create": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(VcfConfig)]),
    "omx_vcf_encoder_load": (c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.POINTER(c_int64), c_int]),
    "omx_vcf_encoder_tokens": (c_int, [c_void_p, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "omx_vcf_encoder_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "omx_vcf_encoder_launches": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "omx_vcf_encoder_scratch_bytes": (c_int, [c_void_p, ctypes.POINTER(ctypes.c_size_t)]),
    "omx_vcf_encoder_debug_read": (c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.c_size_t]),
    "omx_vcf_encoder_destroy": (c_int, [c_void_p]),
}
for _n, (_r, _a) in AUDIO_SIGNATURES.items():
    _f = getattr(lib, _n)
    _f.restype, _f.argtypes = _r, _a


class MelFrontend:
    def __init__(self, sample_rate=16000, n_mels=80, n_fft=400, hop_length=160, lfr_m=7, lfr_n=6):
        require_device()
        self.cfg = MelConfig(sample_rate, n_mels, n_fft, hop_length, lfr_m, lfr_n)
        self._h = c_void_p()
        check(lib.omx_mel_frontend_create(ctypes.byref(self._h), ctypes.byref(self.cfg)))

    def __del__(self):
        if sys is not None and not sys.is_finalizing() and getattr(self, "_h", None) is not None and self._h.value:
            lib.omx_mel_frontend_destroy(self._h)
            self._h = c_void_p()

    def set_cmvn(self, addshift, rescale) -> None:
        a = np.ascontiguousarray(addshift, np.float32)
        r = np.ascontiguousarray(rescale, np.float32)
        check(lib.omx_mel_frontend_set_cmvn(self._h, a.ctypes.data, r.ctypes.data, a.size))

    def frames(self, n_samples: int):
        nf, nl = c_int(), c_int()
        check(lib.omx_mel_frontend_frames(self._h, n_samples, ctypes.byref(nf), ctypes.byref(nl)))
        return nf.value, nl.value

    def forward(self, audio, return_intermediates: bool = False):
        """audio: Tensor f32 [n] (device) or a numpy array.  Returns Tensor [1, T', lfr_m*n_mels] f32."""
        a = audio if isinstance(audio, Tensor) else Tensor.from_numpy(np.asarray(audio, np.float32).ravel(), "f32")
        n = a.size
        nf, nl = self.frames(n)
        dim = self.cfg.lfr_m * self.cfg.n_mels
        feats = Tensor((1, nl, dim), "f32")
        logmel = Tensor((nf, self.cfg.n_mels), "f32") if return_intermediates else None
        power = Tensor((nf, self.cfg.n_fft // 2 + 1), "f32") if return_intermediates else None
        check(lib.omx_mel_frontend_forward(self._h, a.ptr, n, feats.ptr, logmel.ptr if logmel else None,
                                           power.ptr if power else None, None))
        return (feats, logmel, power) if return_intermediates else feats


class WhisperMelFrontend:
    """qwen3-asr-mlx/src/audio.rs:32-128 (`MelFrontend::{new, compute_mel_spectrogram}`): WhisperFeatureExtractor-compatible
    log-mel, [n_mels, n_frames] float32 on the device."""

    def __init__(self, sample_rate=16000, n_mels=128, n_fft=400, hop_length=160):
        require_device()
        self.sample_rate, self.n_mels, self.n_fft, self.hop_length = sample_rate, n_mels, n_fft, hop_length
        self._h = c_void_p()
        check(lib.omx_whisper_mel_create(ctypes.byref(self._h), sample_rate, n_mels, n_fft, hop_length))

    def __del__(self):
        if sys is not None and not sys.is_finalizing() and getattr(self, "_h", None) is not None and self._h.value:
            lib.omx_mel_frontend_destroy(self._h)
            self._h = c_void_p()

    def compute_mel_spectrogram(self, samples) -> Tensor:
        a = samples if isinstance(samples, Tensor) else Tensor.from_numpy(np.asarray(samples, np.float32).ravel(), "f32")
        nf = c_int()
        check(lib.omx_whisper_mel_frames(self._h, a.size, ctypes.byref(nf)))
        out = Tensor((self.n_mels, nf.value), "f32")
        check(lib.omx_whisper_mel_forward(self._h, a.ptr, a.size, out.ptr, None))
        return out


class AudioEncoder:
    """qwen3-asr-mlx/src/encoder.rs:254-458 (`AudioEncoder::{new, forward_encoder}`) in float32 on the device: mel [n_mels, n_frames]
    -> audio rows [N, output_dim].  Keyword names are config.json's `audio_config` keys, defaults the reference's (:43-53)."""

    def __init__(self, num_mel_bins=128, encoder_layers=24, encoder_attention_heads=16, encoder_ffn_dim=4096, d_model=1024,
                 max_source_positions=1500, n_window=50, output_dim=2048, n_window_infer=800, downsample_hidden_size=480, **_ignored):
        require_device()
        self.cfg = AudioEncoderConfig(num_mel_bins, encoder_layers, encoder_attention_heads, encoder_ffn_dim, d_model, max_source_positions,
                                      n_window, output_dim, n_window_infer, downsample_hidden_size)
        self._h = c_void_p()
        check(lib.omx_qwen3_asr_encoder_create(ctypes.byref(self._h), ctypes.byref(self.cfg)))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.omx_qwen3_asr_encoder_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        if sys is not None and not sys.is_finalizing():
            self.close()

    def load_weights(self, weights) -> None:
        """{key behind "audio_tower.": array}; bf16 checkpoints arrive widened (loader.read_safetensors' Bf16Bits are widened here)."""
        for name, arr in weights.items():
            if type(arr).__name__ == "Bf16Bits":
                arr = (np.asarray(arr).astype(np.uint32) << np.uint32(16)).view(np.float32)
            a = np.ascontiguousarray(arr, dtype=np.float32)
            shape = (c_int64 * a.ndim)(*a.shape)
            check(lib.omx_qwen3_asr_encoder_load(self._h, name.encode(), a.ctypes.data, shape, a.ndim))

    def tokens(self, n_frames: int) -> int:
        n = c_int()
        check(lib.omx_qwen3_asr_encoder_tokens(self._h, int(n_frames), ctypes.byref(n)))
        return n.value

    def debug_read(self, name: str, shape) -> np.ndarray:
        """A stage of the last forward ("x1" / "x2" / "x3" [chunks, f, t, ds], "h" [N, d_model]) as float32 (test hook)."""
        out = np.empty(shape, np.float32)
        check(lib.omx_qwen3_asr_encoder_debug_read(self._h, name.encode(), out.ctypes.data, out.size))
        return out

    def forward(self, mel) -> Tensor:
        m = mel if isinstance(mel, Tensor) else Tensor.from_numpy(np.asarray(mel, np.float32), "f32")
        if len(m.shape) != 2 or m.shape[0] != self.cfg.n_mels:
            raise OmxError(f"ShapeMismatch: mel has shape {m.shape}, the tower expects [{self.cfg.n_mels}, n_frames]")
        out = Tensor((self.tokens(m.shape[1]), self.cfg.output_dim), "f32")
        check(lib.omx_qwen3_asr_encoder_forward(self._h, m.ptr, m.shape[1], out.ptr, None))
        return out


def _seg_offsets(lengths):
    """row offsets int[n + 1] of utterances of the given row counts"""
    off = np.zeros(len(lengths) + 1, np.int64)
    off[1:] = np.cumsum(np.asarray(lengths, np.int64))
    return (c_int * len(off))(*[int(v) for v in off]), int(off[-1])


class FunASRNanoEncoder:
    """funasr-nano-mlx's audio tower in float32 on the device: SenseVoiceEncoder::forward (sensevoice_encoder.rs:453-478) followed by
    AudioAdaptor::forward (adaptor.rs:247-261), over up to 8 utterances in one pass.  Keyword names are config.yaml's
    `audio_encoder_conf` / `audio_adaptor_conf` keys, defaults the reference's."""

    MAX_UTTERANCES, MAX_ROWS = 8, 512

    def __init__(self, lfr_dim=560, output_size=512, attention_heads=4, linear_units=2048, num_blocks=50, tp_blocks=20, kernel_size=11,
                 encoder_dim=512, ffn_dim=2048, llm_dim=1024, n_layer=2, **_ignored):
        require_device()
        self.cfg = FunASRNanoEncoderConfig(lfr_dim, output_size, attention_heads, linear_units, num_blocks, tp_blocks, kernel_size,
                                           encoder_dim, ffn_dim, llm_dim, n_layer)
        self._h = c_void_p()
        check(lib.omx_funasr_nano_encoder_create(ctypes.byref(self._h), ctypes.byref(self.cfg)))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.omx_funasr_nano_encoder_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        if sys is not None and not sys.is_finalizing():
            self.close()

    def load_weights(self, weights) -> None:
        """{key after the reference's key map ("encoder.…" / "adaptor.…"): array}; bf16 tensors (loader's Bf16Bits) are widened here."""
        for name, arr in weights.items():
            if type(arr).__name__ == "Bf16Bits":
                arr = (np.asarray(arr).astype(np.uint32) << np.uint32(16)).view(np.float32)
            a = np.ascontiguousarray(arr, dtype=np.float32)
            shape = (c_int64 * a.ndim)(*a.shape)
            check(lib.omx_funasr_nano_encoder_load(self._h, name.encode(), a.ctypes.data, shape, a.ndim))

    def debug_read(self, name: str, shape) -> np.ndarray:
        """A stage of the last forward ("pos", "after_norm", "tp_norm", "linear2") as float32 (test hook)."""
        out = np.empty(shape, np.float32)
        check(lib.omx_funasr_nano_encoder_debug_read(self._h, name.encode(), out.ctypes.data, out.size))
        return out

    def forward(self, lfr_rows, lengths=None) -> Tensor:
        """lfr_rows: f32 [sum T, lfr_dim] (Tensor or numpy), the utterances' LFR rows stacked; lengths: their row counts (default: one
        utterance).  -> Tensor f32 [sum T, llm_dim], utterance u at rows [sum(lengths[:u]), sum(lengths[:u + 1]))."""
        x = lfr_rows if isinstance(lfr_rows, Tensor) else Tensor.from_numpy(np.ascontiguousarray(lfr_rows, np.float32), "f32")
        if len(x.shape) != 2 or x.shape[1] != self.cfg.lfr_dim:
            raise OmxError(f"ShapeMismatch: lfr_rows has shape {x.shape}, the tower expects [rows, {self.cfg.lfr_dim}]")
        lengths = [x.shape[0]] if lengths is None else [int(v) for v in lengths]
        seg, total = _seg_offsets(lengths)
        if total != x.shape[0]:
            raise OmxError(f"ShapeMismatch: the utterances hold {total} rows, lfr_rows has {x.shape[0]}")
        out = Tensor((max(total, 1), self.cfg.llm_dim), "f32")
        check(lib.omx_funasr_nano_encoder_forward(self._h, x.ptr, seg, len(lengths), out.ptr, None))
        return out


def segment_attention_f32(qkv: Tensor, heads: int, lengths) -> Tensor:
    """The tower's attention alone (omx_segment_attention_f32): qkv f32 [sum T, ld >= 3 * heads * 128] holding q | k | v side by side from
    column 0, utterances of `lengths` rows stacked; -> [sum T, heads * 128]."""
    d = heads * 128
    ld = qkv.shape[1]
    seg, total = _seg_offsets(lengths)
    out = Tensor((max(total, 1), d), "f32")
    check(lib.omx_segment_attention_f32(out.ptr, qkv.ptr, qkv.ptr + 4 * d, qkv.ptr + 8 * d, ld, ld, d, seg, len(lengths), heads, None))
    return out


def window_attention_f32(qkv: Tensor, heads: int, window: int, n: int = None) -> Tensor:
    """The tower's attention alone (omx_window_attention_f32): qkv f32 [N, ld >= 3 * heads * 64] holding q | k | v side by side from
    column 0; -> [N, heads * 64]."""
    d = heads * 64
    N, ld = (qkv.shape[0] if n is None else n), qkv.shape[1]
    out = Tensor((N, d), "f32")
    check(lib.omx_window_attention_f32(out.ptr, d, qkv.ptr, qkv.ptr + 4 * d, qkv.ptr + 8 * d, ld, N, heads, window, None))
    return out


class SenseVoiceMelFrontend:
    """funasr-nano-mlx/src/audio.rs:44-157 (`AudioConfig`, `MelFrontend::{new, compute_mel_spectrogram}`): the Fun-ASR-Nano / SenseVoice
    log-mel, [1, n_mels, n_frames] float32 on the device; `apply_lfr` (:345-412) stacks it to [1, ceil(T / n), m * n_mels]."""

    def __init__(self, sample_rate=16000, n_mels=80, n_fft=400, hop_length=160, max_length=30.0):
        require_device()
        self.sample_rate, self.n_mels, self.n_fft, self.hop_length, self.max_length = sample_rate, n_mels, n_fft, hop_length, max_length
        self.n_freqs = n_fft // 2 + 1
        self._h = c_void_p()
        check(lib.omx_sensevoice_mel_create(ctypes.byref(self._h), sample_rate, n_mels, n_fft, hop_length, max_length))

    def __del__(self):
        if sys is not None and not sys.is_finalizing() and getattr(self, "_h", None) is not None and self._h.value:
            lib.omx_mel_frontend_destroy(self._h)
            self._h = c_void_p()

    def compute_mel_spectrogram(self, samples) -> Tensor:
        a = samples if isinstance(samples, Tensor) else Tensor.from_numpy(np.asarray(samples, np.float32).ravel(), "f32")
        if a.size == 0:
            check(lib.omx_sensevoice_mel_frames(self._h, 0, ctypes.byref(c_int())))      # raises the reference's "samples are empty"
        nf = c_int()
        check(lib.omx_sensevoice_mel_frames(self._h, a.size, ctypes.byref(nf)))
        out = Tensor((1, self.n_mels, nf.value), "f32")
        check(lib.omx_sensevoice_mel_forward(self._h, a.ptr, a.size, out.ptr, None))
        return out


def apply_lfr(mel: Tensor, lfr_m: int, lfr_n: int) -> Tensor:
    """funasr-nano-mlx/src/audio.rs:345-412: [1, n_mels, n_frames] -> [1, ceil(n_frames / lfr_n), n_mels * lfr_m] (device to device; the
    reference copies the spectrogram to the host and back for this)."""
    if len(mel.shape) != 3 or mel.shape[0] != 1:
        raise ValueError(f"apply_lfr: expected [1, n_mels, n_frames], got {mel.shape}")
    _, n_mels, n_frames = mel.shape
    out = Tensor((1, (n_frames + lfr_n - 1) // lfr_n, n_mels * lfr_m), "f32")
    check(lib.omx_apply_lfr(out.ptr, mel.ptr, n_mels, n_frames, lfr_m, lfr_n, None))
    return out


def resample_device(samples: Tensor, src_rate: int, target_rate: int) -> Tensor:
    """audio::resample on a device tensor (f32 [n]) -> device tensor (f32 [m])."""
    n = samples.size
    cap = int(lib.omx_resample_len(n, src_rate, target_rate))
    out = Tensor((max(cap, 1),), "f32")
    m = c_int64()
    check(lib.omx_resample_sinc(samples.ptr if n else None, n, src_rate, target_rate, out.ptr, cap, ctypes.byref(m), None))
    if m.value == out.shape[0]:
        return out
    return Tensor((m.value,), "f32", ptr=out.ptr, owner=out)      # a prefix view of the allocation (short inputs give fewer samples)


def resample(samples, src_rate: int, target_rate: int) -> np.ndarray:
    """`audio::resample` (mlx-rs-core/src/audio.rs:178-277): host samples in, host samples out (float32), windowed-sinc interpolation with
    the reference's rubato configuration, evaluated on the GPU (csrc/resample.hip)."""
    x = np.ascontiguousarray(np.asarray(samples, np.float32).ravel())
    if src_rate == target_rate or x.size == 0:              # :179-181
        return x.copy()
    require_device()
    cap = int(lib.omx_resample_len(x.size, src_rate, target_rate))
    src = Tensor.from_numpy(x, "f32")
    out = Tensor((max(cap, 1),), "f32")
    m = c_int64()
    check(lib.omx_resample_sinc(src.ptr, x.size, src_rate, target_rate, out.ptr, cap, ctypes.byref(m), None))
    return out.numpy().ravel()[: m.value].copy()


# ---- WAV container, host side (mlx-rs-core/src/audio.rs:46-163 `load_wav`, :285-326 `save_wav`) ----

def load_wav(path):
    """-> (mono float32 samples in [-1, 1], sample_rate).  PCM 16 / 24 bit and 32-bit float; unknown chunks are skipped;
    multi-channel audio is averaged to mono; errors as the reference's ("Not a RIFF file", "Not a WAVE file",
    "Unsupported bits per sample: N")."""
    import struct
    with open(path, "rb") as fh:
        buf = fh.read()
    if buf[:4] != b"RIFF":
        raise ValueError("Not a RIFF file")
    if buf[8:12] != b"WAVE":
        raise ValueError("Not a WAVE file")
    pos, sample_rate, bits, channels, data = 12, 0, 16, 1, b""
    while pos + 8 <= len(buf):
        chunk_id = buf[pos:pos + 4]
        (size,) = struct.unpack_from("<I", buf, pos + 4)
        pos += 8
        if chunk_id == b"fmt ":
            _fmt, channels, sample_rate, _rate, _align, bits = struct.unpack_from("<HHIIHH", buf, pos)
        elif chunk_id == b"data":
            data = buf[pos:pos + size]
            break
        pos += size
    if bits == 16:
        x = np.frombuffer(data, "<i2", len(data) // 2).astype(np.float32) / np.float32(32768.0)
    elif bits == 24:
        b3 = np.frombuffer(data, np.uint8, len(data) // 3 * 3).reshape(-1, 3).astype(np.int32)
        v = ((b3[:, 0] << 8) | (b3[:, 1] << 16) | (b3[:, 2] << 24)) >> 8          # sign-extending shift, as the Rust
        x = v.astype(np.float32) / np.float32(8388608.0)
    elif bits == 32:
        x = np.frombuffer(data, "<f4", len(data) // 4).astype(np.float32)
    else:
        raise ValueError(f"Unsupported bits per sample: {bits}")
    if channels > 1:
        x = x[:x.size // channels * channels].reshape(-1, channels)
        acc = np.zeros(x.shape[0], np.float32)
        for c in range(channels):
            acc = acc + x[:, c]
        x = acc / np.float32(channels)
    return x.astype(np.float32), int(sample_rate)


def save_wav(samples, sample_rate: int, path) -> None:
    """16-bit PCM mono; sample -> (clamp(x, -1, 1) * 32767) truncated toward zero (`as i16`)."""
    import struct
    x = np.clip(np.asarray(samples, np.float32).ravel(), np.float32(-1.0), np.float32(1.0))
    pcm = np.trunc(x * np.float32(32767.0)).astype("<i2")
    data = pcm.tobytes()
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE")
        fh.write(b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, sample_rate, sample_rate * 2, 2, 16))
        fh.write(b"data" + struct.pack("<I", len(data)) + data)
