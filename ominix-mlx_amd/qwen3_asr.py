"""Qwen3-ASR on the device (qwen3-asr-mlx/src/model.rs): Whisper log-mel -> audio tower (float32, csrc/audio_encoder.hip) -> the
tower's rows over the <|audio_pad|> span of the prompt (Model.prefill(embeds=, embeds_at=)) -> greedy / sampled decode of the Qwen3
text decoder -> text.  Host logic only; every hot path is a device call of audio.py / engine.py."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import OmxError

AUDIO_PREFIX = "audio_tower."
DEFAULT_EOS = (151645, 151643)          # <|im_end|>, <|endoftext|> (model.rs:568-570)


@dataclass
class Qwen3ASRConfig:
    """Qwen3ASRConfig (model.rs:33-129).  audio_config / text_config keep config.json's keys (AudioEncoder / engine.Model keywords)."""
    audio_config: dict = field(default_factory=dict)
    text_config: dict = field(default_factory=dict)
    audio_token_id: int = 151676
    audio_start_token_id: int = 151669
    audio_end_token_id: int = 151670
    support_languages: List[str] = field(default_factory=list)
    quantization: Optional[dict] = None

    @staticmethod
    def from_config_json(value: dict) -> "Qwen3ASRConfig":
        """model.rs:76-129: the model's fields sit under `thinker_config` when it is there; `quantization` and `support_languages`
        are read at the top level."""
        thinker = value.get("thinker_config", value)

        def as_int(key, default):
            v = thinker.get(key)
            return int(v) if isinstance(v, int) and not isinstance(v, bool) else default

        langs = value.get("support_languages")
        q = value.get("quantization")
        return Qwen3ASRConfig(audio_config=dict(thinker.get("audio_config") or {}), text_config=dict(thinker.get("text_config") or {}),
                              audio_token_id=as_int("audio_token_id", 151676), audio_start_token_id=as_int("audio_start_token_id", 151669),
                              audio_end_token_id=as_int("audio_end_token_id", 151670),
                              support_languages=[s for s in langs if isinstance(s, str)] if isinstance(langs, list) else [],
                              quantization=dict(q) if isinstance(q, dict) else None)

    def text_model_args(self) -> dict:
        """keywords of engine.Model from text_config (the reference's QwenConfig: tied head, q/k norms, standard RoPE)"""
        c = self.text_config
        for key in ("hidden_size", "num_hidden_layers", "intermediate_size", "num_attention_heads", "vocab_size"):
            if key not in c:
                raise OmxError(f"InvalidConfig: qwen3-asr text_config lacks {key}")
        return dict(hidden_size=c["hidden_size"], num_hidden_layers=c["num_hidden_layers"], intermediate_size=c["intermediate_size"],
                    num_attention_heads=c["num_attention_heads"], num_key_value_heads=c.get("num_key_value_heads", c["num_attention_heads"]),
                    head_dim=c.get("head_dim") or c["hidden_size"] // c["num_attention_heads"], vocab_size=c["vocab_size"],
                    rms_norm_eps=c.get("rms_norm_eps", 1e-6), rope_theta=c.get("rope_theta", 1e6),
                    tie_word_embeddings=c.get("tie_word_embeddings", True), rope_scaling=c.get("rope_scaling"), quantization=self.quantization)


def split_weights(weights: Dict[str, np.ndarray]) -> Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray]]:
    """(tower tensors with "audio_tower." taken off, text tensors: "model.*" and "lm_head.*") -- model.rs:311-312, 457-462"""
    tower = {k[len(AUDIO_PREFIX):]: v for k, v in weights.items() if k.startswith(AUDIO_PREFIX)}
    text = {k: v for k, v in weights.items() if k.startswith(("model.", "lm_head."))}
    return tower, text


def prompt_text(num_audio_tokens: int, language: str) -> str:
    """the exact template of build_prompt (model.rs:705-709)"""
    return ("<|im_start|>system\n<|im_end|>\n<|im_start|>user\n<|audio_start|>" + "<|audio_pad|>" * int(num_audio_tokens) +
            "<|audio_end|><|im_end|>\n<|im_start|>assistant\nlanguage " + language + "<asr_text>")


def encode(tokenizer, text: str) -> np.ndarray:
    enc = tokenizer.encode(text, add_special_tokens=False)
    return np.asarray(getattr(enc, "ids", enc), dtype=np.uint32)


def audio_span(ids: Sequence[int], audio_token_id: int, n_rows: int) -> int:
    """Index of the first <|audio_pad|>.  The reference silently takes the first-to-last pad span whatever its length
    (model.rs:737-768); here the pads must be one run of exactly the tower's row count."""
    ids = np.asarray(ids)
    at = np.nonzero(ids == audio_token_id)[0]
    if at.size != n_rows:
        raise OmxError(f"qwen3-asr: the prompt holds {at.size} <|audio_pad|> ids but the tower made {n_rows} rows")
    if n_rows and at[-1] - at[0] + 1 != n_rows:
        raise OmxError("qwen3-asr: the <|audio_pad|> ids of the prompt are not one contiguous span")
    return int(at[0]) if n_rows else 0


def generate_ids(model, first: int, max_tokens: int, eos_ids: Iterable[int], chunk: int = 16) -> List[int]:
    """The reference's loop (model.rs:794-810) over a model that has just been prefilled: `first` is the prompt's sampled token; a token
    is emitted unless it is an EOS id or the tenth equal token in a row (the stopping token is not emitted); at most max_tokens.
    Tokens are fetched `chunk` decode steps at a time."""
    eos = set(int(t) for t in eos_ids)
    out: List[int] = []
    recent: List[int] = []
    pending: List[int] = []
    tok = int(first)
    for _ in range(max_tokens):
        if tok in eos:
            break
        recent.append(tok)
        if len(recent) > 10:
            recent.pop(0)
        if len(recent) >= 10 and all(t == tok for t in recent):
            break
        out.append(tok)
        if not pending:
            pending = [int(t) for t in model.decode(chunk)]
        tok = pending.pop(0)
    return out


def parse_eos_tokens(model_dir: str) -> List[int]:
    """model.rs:539-573: the id of tokenizer_config.json's `eos_token` from `added_tokens_decoder`; the Qwen3 defaults otherwise"""
    path = os.path.join(model_dir, "tokenizer_config.json")
    ids: List[int] = []
    try:
        with open(path) as f:
            cfg = json.load(f)
        eos = cfg.get("eos_token")
        eos = eos.get("content") if isinstance(eos, dict) else eos
        for tid, entry in (cfg.get("added_tokens_decoder") or {}).items():
            if isinstance(entry, dict) and entry.get("content") == eos and int(tid) not in ids:
                ids.append(int(tid))
    except (OSError, ValueError):
        pass
    return ids or list(DEFAULT_EOS)


def read_checkpoint(model_dir: str):
    """The device-free half of load: (config, tower tensors, text tensors, eos ids)."""
    from . import loader
    with open(os.path.join(model_dir, "config.json")) as f:
        config = Qwen3ASRConfig.from_config_json(json.load(f))
    tower, text = split_weights(loader.load_all_weights(model_dir))
    if not tower:
        raise OmxError(f"{model_dir}: no audio_tower.* tensors (not a Qwen3-ASR checkpoint)")
    return config, tower, text, parse_eos_tokens(model_dir)


def read_wav(path: str) -> Tuple[np.ndarray, int]:
    """16-bit PCM WAV -> (mono float32 samples, sample rate)"""
    import wave
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2:
            raise OmxError(f"{path}: {8 * w.getsampwidth()}-bit samples (16-bit PCM only)")
        rate, ch = w.getframerate(), w.getnchannels()
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.float32) / 32768.0
    return (pcm.reshape(-1, ch).mean(axis=1) if ch > 1 else pcm).astype(np.float32), rate


class Qwen3ASR:
    """Qwen3ASR (model.rs:148-350): `load(model_dir)`, `transcribe(path, language)`, `transcribe_samples(samples, language, ...)`."""

    def __init__(self, config: Qwen3ASRConfig, model, encoder, frontend, tokenizer, eos_ids=DEFAULT_EOS):
        self.config, self.model, self.encoder, self.frontend, self.tokenizer = config, model, encoder, frontend, tokenizer
        self.eos_ids = [int(t) for t in eos_ids]
        self.last_times = {}

    @staticmethod
    def load(model_dir: str, max_context: int = 4096) -> "Qwen3ASR":
        from . import audio, engine, generate
        config, tower, text, eos = read_checkpoint(model_dir)
        args = dict(config.text_model_args(), max_context=max_context)
        q = args.get("quantization")
        if q is not None and any(k.endswith(".scales") and np.asarray(v).dtype == np.float16 for k, v in text.items()):
            args["quantization"] = dict(q, scales_dtype="float16")
        model = engine.Model(**args)
        model.load_weights({k: v for k, v in text.items() if not (args["tie_word_embeddings"] and k.startswith("lm_head."))})
        encoder = audio.AudioEncoder(**config.audio_config)      # never quantised (model.rs:305): widened to float32
        encoder.load_weights(tower)
        frontend = audio.WhisperMelFrontend(n_mels=config.audio_config.get("num_mel_bins", 128))
        return Qwen3ASR(config, model, encoder, frontend, generate.load_tokenizer(model_dir), eos)

    def transcribe_ids(self, samples, language: str = "English", temperature: float = 0.0, max_tokens: int = 512, seed: int = 0,
                       chunk: int = 16) -> List[int]:
        """transcribe_samples_with_config (model.rs:673-698) up to the token ids."""
        import time
        t0 = time.perf_counter()
        mel = self.frontend.compute_mel_spectrogram(np.asarray(samples, dtype=np.float32))
        rows = self.encoder.forward(mel)
        n = rows.shape[0]
        ids = encode(self.tokenizer, prompt_text(n, language))
        at = audio_span(ids, self.config.audio_token_id, n)
        self.model.reset()
        self.model.set_sampler(float(temperature), seed)
        first = self.model.prefill(ids, embeds=rows, embeds_at=at)
        t1 = time.perf_counter()
        out = generate_ids(self.model, first, max_tokens, self.eos_ids, chunk)
        self.last_times = {"frames": mel.shape[1], "audio_rows": n, "prompt_rows": int(ids.size), "to_first_token_s": t1 - t0,
                           "prompt_pass_ms": self.model.last_prefill_ms(), "decode_s": time.perf_counter() - t1, "tokens": len(out)}
        return out

    def transcribe_samples(self, samples, language: str = "English", temperature: float = 0.0, max_tokens: int = 512, seed: int = 0) -> str:
        return self.tokenizer.decode(self.transcribe_ids(samples, language, temperature, max_tokens, seed), skip_special_tokens=True)

    def transcribe(self, path: str, language: str = "English") -> str:
        samples, rate = read_wav(path)
        if rate != 16000:
            raise OmxError(f"{path}: {rate} Hz (16 kHz expected; resample first, audio.py has the device resampler)")
        return self.transcribe_samples(samples, language)
