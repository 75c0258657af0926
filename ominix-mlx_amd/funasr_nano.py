"""Fun-ASR-Nano on the device (funasr-nano-mlx/src/model.rs): SenseVoice log-mel -> LFR rows -> SenseVoice tower + adaptor (float32,
csrc/sensevoice_encoder.hip, up to 8 utterances in one pass) -> the adapted rows between <|startofspeech|> and <|endofspeech|> of a ChatML
prompt (prefill(embeds=, embeds_at=)) -> greedy / sampled decode of the Qwen3-0.6B decoder -> text.  One utterance goes through
engine.Model; several go through one engine.Batch of up to 8 slots (the reference loops over them one at a time, model.rs:463-476).
Host logic only; every hot path is a device call of audio.py / engine.py."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import OmxError

MAX_GROUP = 8                           # utterances per tower pass and slots per Batch
JOINT_TOWER_DEFAULT = True              # the joint pass against the per-utterance loop, measured
LFR_M, LFR_N = 7, 6                     # model.rs:395
DEFAULT_SYSTEM = "You are a helpful assistant."
DEFAULT_INSTRUCTION = "语音转写成中文："
SPECIAL_NAMES = {"im_start": "<|im_start|>", "im_end": "<|im_end|>", "eos": "<|endoftext|>", "speech_start": "<|startofspeech|>",
                 "speech_end": "<|endofspeech|>"}
ENCODER_DEFAULTS = dict(output_size=512, attention_heads=4, linear_units=2048, num_blocks=50, tp_blocks=20, kernel_size=11)   # sensevoice_encoder.rs:56-69
ADAPTOR_DEFAULTS = dict(encoder_dim=512, ffn_dim=2048, llm_dim=1024, n_layer=2)                                                # adaptor.rs:43-53

# map_safetensors_key (model.rs:350-374), in its order
KEY_MAP = ((".attn.qkv.", ".self_attn.linear_q_k_v."), (".attn.out.", ".self_attn.linear_out."), (".attn.fsmn.", ".self_attn.fsmn."),
           (".ffn.w1.", ".feed_forward.w_1."), (".ffn.w2.", ".feed_forward.w_2."), (".attn.q.", ".self_attn.linear_q."),
           (".attn.k.", ".self_attn.linear_k."), (".attn.v.", ".self_attn.linear_v."), (".attn.q_proj.", ".self_attn.q_proj."),
           (".attn.k_proj.", ".self_attn.k_proj."), (".attn.v_proj.", ".self_attn.v_proj."), (".attn.o_proj.", ".self_attn.o_proj."),
           (".attn.q_norm.", ".self_attn.q_norm."), (".attn.k_norm.", ".self_attn.k_norm."))


def map_key(key: str) -> str:
    for old, new in KEY_MAP:
        key = key.replace(old, new)
    return key


def llm_key(key: str) -> Optional[str]:
    """a mapped key of the `llm.` member under the name engine.Model takes (None: not the decoder's)"""
    if not key.startswith("llm."):
        return None
    rest = key[4:]
    return rest if rest.startswith("lm_head.") else "model." + rest


def split_weights(weights: Dict[str, np.ndarray]) -> Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray], List[str]]:
    """(tower tensors "encoder.*" / "adaptor.*", decoder tensors under engine.Model's names, keys that are neither)"""
    tower, text, other = {}, {}, []
    for raw, v in weights.items():
        k = map_key(raw)
        if k.startswith(("encoder.", "adaptor.")):
            tower[k] = v
        elif llm_key(k) is not None:
            text[llm_key(k)] = v
        else:
            other.append(raw)
    return tower, text, other


def parse_config(yaml_text: Optional[str]) -> dict:
    """load_config (model.rs:214-299): integer fields of `audio_encoder_conf` / `audio_adaptor_conf`, the reference's defaults for what
    is absent (a section, a field, the file); lfr_dim is 80 mels x 7.  -> keywords of audio.FunASRNanoEncoder."""
    import yaml
    doc = yaml.safe_load(yaml_text) if yaml_text else None
    doc = doc if isinstance(doc, dict) else {}

    def section(name, defaults):
        conf = doc.get(name)
        conf = conf if isinstance(conf, dict) else {}
        return {k: (int(conf[k]) if isinstance(conf.get(k), int) and not isinstance(conf.get(k), bool) else d) for k, d in defaults.items()}

    return dict(lfr_dim=80 * LFR_M, **section("audio_encoder_conf", ENCODER_DEFAULTS), **section("audio_adaptor_conf", ADAPTOR_DEFAULTS))


def tower_weight_shapes(cfg: dict) -> Dict[str, tuple]:
    """every tensor of the tower and the adaptor (mapped keys) with the shape the config implies"""
    dim, ffn, llm, k = cfg["output_size"], cfg["linear_units"], cfg["llm_dim"], cfg["kernel_size"]
    layers = (["encoder.encoders0.0"] + [f"encoder.encoders.{i}" for i in range(cfg["num_blocks"] - 1)] +
              [f"encoder.tp_encoders.{i}" for i in range(cfg["tp_blocks"])])
    s: Dict[str, tuple] = {}

    def linear(name, n_out, n_in):
        s[name + ".weight"], s[name + ".bias"] = (n_out, n_in), (n_out,)

    def norm(name, n):
        s[name + ".weight"] = s[name + ".bias"] = (n,)

    for i, p in enumerate(layers):
        d_in = cfg["lfr_dim"] if i == 0 else dim
        norm(p + ".norm1", d_in), norm(p + ".norm2", dim)
        linear(p + ".self_attn.linear_q_k_v", 3 * dim, d_in), linear(p + ".self_attn.linear_out", dim, dim)
        s[p + ".self_attn.fsmn.weight"] = (dim, 1, k)
        linear(p + ".feed_forward.w_1", ffn, dim), linear(p + ".feed_forward.w_2", dim, ffn)
    norm("encoder.after_norm", dim), norm("encoder.tp_norm", dim)
    linear("adaptor.linear1", cfg["ffn_dim"], cfg["encoder_dim"]), linear("adaptor.linear2", llm, cfg["ffn_dim"])
    for i in range(cfg["n_layer"]):
        p = f"adaptor.blocks.{i}"
        for n in ("linear_q", "linear_k", "linear_v", "linear_out"):
            linear(f"{p}.self_attn.{n}", llm, llm)
        norm(p + ".norm1", llm), norm(p + ".norm2", llm)
        linear(p + ".feed_forward.w_1", 256, llm), linear(p + ".feed_forward.w_2", llm, 256)     # adaptor.rs:227
    return s


def text_model_args(c: dict) -> dict:
    """keywords of engine.Model from Qwen3-0.6B/config.json"""
    for key in ("hidden_size", "num_hidden_layers", "intermediate_size", "num_attention_heads", "vocab_size"):
        if key not in c:
            raise OmxError(f"InvalidConfig: funasr-nano Qwen3-0.6B/config.json lacks {key}")
    return dict(hidden_size=c["hidden_size"], num_hidden_layers=c["num_hidden_layers"], intermediate_size=c["intermediate_size"],
                num_attention_heads=c["num_attention_heads"], num_key_value_heads=c.get("num_key_value_heads", c["num_attention_heads"]),
                head_dim=c.get("head_dim") or c["hidden_size"] // c["num_attention_heads"], vocab_size=c["vocab_size"],
                rms_norm_eps=c.get("rms_norm_eps", 1e-6), rope_theta=c.get("rope_theta", 1e6),
                tie_word_embeddings=c.get("tie_word_embeddings", True), rope_scaling=c.get("rope_scaling"))


@dataclass
class SamplingConfig:
    """SamplingConfig (model.rs:77-100); temperature 0 = greedy"""
    temperature: float = 0.0
    top_k: int = 0
    top_p: float = 1.0
    repetition_penalty: float = 1.0
    max_tokens: int = 256
    seed: int = 0


@dataclass
class Markers:
    """ids of the special tokens, looked up by name in the model's tokenizer (SPECIAL_NAMES)"""
    im_start: int
    im_end: int
    eos: int
    speech_start: int
    speech_end: int

    @staticmethod
    def from_tokenizer(tokenizer) -> "Markers":
        ids = {}
        for field_name, text in SPECIAL_NAMES.items():
            tid = tokenizer.token_to_id(text)
            if tid is None:
                raise OmxError(f"funasr-nano: the tokenizer has no {text} token")
            ids[field_name] = int(tid)
        return Markers(**ids)


def _encode(tokenizer, text: str) -> List[int]:
    enc = tokenizer.encode(text, add_special_tokens=False)
    return [int(t) for t in getattr(enc, "ids", enc)]


@dataclass
class Prompt:
    """the ids around the audio span: prefix ... <|startofspeech|> {rows} <|endofspeech|> suffix"""
    prefix: List[int]
    suffix: List[int]
    markers: Markers = field(repr=False, default=None)

    def ids(self, n_rows: int) -> Tuple[np.ndarray, int]:
        """(prompt ids with placeholder id 0 under the rows, index of the first row) -- model.rs:583-601"""
        m = self.markers
        ids = self.prefix + [m.speech_start] + [0] * int(n_rows) + [m.speech_end] + self.suffix
        return np.asarray(ids, dtype=np.uint32), len(self.prefix) + 1


def build_prompt(tokenizer, markers: Markers, system: Optional[str] = None, instruction: Optional[str] = None) -> Prompt:
    """The ChatML form of generate_text_with_config (model.rs:543-592):
        <|im_start|>system\\n{system}<|im_end|>\\n<|im_start|>user\\n{instruction}<|startofspeech|>{AUDIO}<|endofspeech|><|im_end|>\\n<|im_start|>assistant\\n
    system / instruction given (transcribe_with_prompt, :1062-1100): the system text is encoded with a newline behind it, as there."""
    m = markers
    custom = system is not None or instruction is not None
    sys_text = (DEFAULT_SYSTEM if system is None else system) + ("\n" if custom else "")
    ins_text = DEFAULT_INSTRUCTION if instruction is None else instruction
    prefix = ([m.im_start] + _encode(tokenizer, "system\n") + _encode(tokenizer, sys_text) + [m.im_end] + _encode(tokenizer, "\n") + [m.im_start] +
              _encode(tokenizer, "user\n") + _encode(tokenizer, ins_text))
    suffix = [m.im_end] + _encode(tokenizer, "\n") + [m.im_start] + _encode(tokenizer, "assistant\n")
    return Prompt(prefix, suffix, m)


class StopRule:
    """The reference's loop conditions (model.rs:628-659), one token at a time: `push(tok)` is True while the token is emitted; False
    once it is <|endoftext|> or <|im_end|>, the tenth equal token in a row, or past max_tokens (the stopping token is not emitted)."""

    def __init__(self, markers: Markers, max_tokens: int = 256):
        self.stop_ids = {int(markers.eos), int(markers.im_end)}
        self.max_tokens = int(max_tokens)
        self.tokens: List[int] = []
        self.recent: List[int] = []
        self.done = self.max_tokens <= 0

    def push(self, tok: int) -> bool:
        tok = int(tok)
        if self.done:
            return False
        if tok in self.stop_ids:
            self.done = True
            return False
        self.recent.append(tok)
        if len(self.recent) > 10:
            self.recent.pop(0)
        if len(self.recent) >= 10 and all(t == tok for t in self.recent):
            self.done = True
            return False
        self.tokens.append(tok)
        if len(self.tokens) >= self.max_tokens:
            self.done = True
        return True


def generate_ids(source, first: int, rule: StopRule, chunk: int = 16) -> List[int]:
    """one sequence: `source.decode(n)` gives the next n tokens after `first`"""
    tok, pending = int(first), []
    while rule.push(tok):
        if rule.done:
            break
        if not pending:
            pending = [int(t) for t in source.decode(chunk)]
        tok = pending.pop(0)
    return rule.tokens


def generate_ids_batch(batch, firsts: Sequence[int], rules: Sequence[StopRule], chunk: int = 8) -> List[List[int]]:
    """slots 0 .. n - 1 of a prefilled Batch: `batch.decode(k, slots)` -> [k, len(slots)].  A slot that has stopped is left out of every
    later decode call; tokens a slot produced after its stop inside a chunk are dropped."""
    live = [s for s, (f, r) in enumerate(zip(firsts, rules)) if r.push(f) and not r.done]
    while live:
        toks = np.asarray(batch.decode(chunk, live)).reshape(chunk, len(live))
        for col, s in enumerate(live):
            for t in toks[:, col]:
                if not rules[s].push(t) or rules[s].done:
                    break
        live = [s for s in live if not rules[s].done]
    return [r.tokens for r in rules]


def groups(n: int, size: int = MAX_GROUP) -> List[range]:
    """n inputs in order, in groups of at most `size`: 11 -> 8 + 3"""
    return [range(i, min(i + size, n)) for i in range(0, n, size)]


def read_checkpoint(model_dir: str):
    """The device-free half of load: (encoder keywords, decoder keywords, tower tensors, decoder tensors)."""
    from . import loader
    path = os.path.join(model_dir, "config.yaml")
    enc_args = parse_config(open(path, encoding="utf-8").read() if os.path.exists(path) else None)
    with open(os.path.join(model_dir, "Qwen3-0.6B", "config.json")) as f:
        text_args = text_model_args(json.load(f))
    st = os.path.join(model_dir, "model.safetensors")
    if not os.path.exists(st):
        raise OmxError(f"ModelLoad: model.safetensors not found at {st}")
    tower, text, _ = split_weights(loader.read_safetensors(st))
    if not tower:
        raise OmxError(f"{model_dir}: no encoder.* / adaptor.* tensors (not a Fun-ASR-Nano checkpoint)")
    return enc_args, text_args, tower, text


class FunASRNano:
    """FunASRNano (model.rs:139-700): `load(model_dir)`, `transcribe(path)`, `transcribe_samples(samples, rate)`,
    `transcribe_with_prompt(path, system, instruction)`, `transcribe_samples_batch([(samples, rate), ...])`."""

    def __init__(self, model, encoder, frontend, tokenizer, prompt: Prompt, joint_tower: Optional[bool] = None, kv_bits: int = 0):
        self.model, self.encoder, self.frontend, self.tokenizer, self.prompt = model, encoder, frontend, tokenizer, prompt
        self.markers = prompt.markers
        # one tower pass over the stacked utterances of a group (OMX_FUNASR_JOINT_TOWER=1), or the same tower once per utterance (=0)
        if joint_tower is None:
            env = os.environ.get("OMX_FUNASR_JOINT_TOWER")
            joint_tower = JOINT_TOWER_DEFAULT if env is None else env != "0"
        self.joint_tower = bool(joint_tower)
        self.kv_bits = int(kv_bits)
        self._batches = {}
        self.last_times = {}

    @staticmethod
    def load(model_dir: str, max_context: int = 2048, kv_bits: int = 0) -> "FunASRNano":
        from . import audio, engine, generate
        enc_args, text_args, tower, text = read_checkpoint(model_dir)
        model = engine.Model(**dict(text_args, max_context=max_context))
        model.load_weights({k: v for k, v in text.items() if not (text_args["tie_word_embeddings"] and k.startswith("lm_head."))})
        encoder = audio.FunASRNanoEncoder(**enc_args)
        encoder.load_weights(tower)
        tokenizer = generate.load_tokenizer(os.path.join(model_dir, "Qwen3-0.6B"))
        markers = Markers.from_tokenizer(tokenizer)
        return FunASRNano(model, encoder, audio.SenseVoiceMelFrontend(), tokenizer, build_prompt(tokenizer, markers), kv_bits=kv_bits)

    # ---- audio -> adapted rows ----

    def lfr_rows(self, samples):
        """16 kHz samples -> device f32 [T, 560] (log-mel, 7 frames stacked every 6)"""
        from . import audio
        mel = self.frontend.compute_mel_spectrogram(np.asarray(samples, dtype=np.float32))
        lfr = audio.apply_lfr(mel, LFR_M, LFR_N)
        return lfr.view((lfr.shape[1], lfr.shape[2]))

    def encode_audio(self, samples_list) -> list:
        """The adapted rows of up to 8 utterances (16 kHz samples each): a list of device Tensors f32 [T_u, llm_dim].  joint_tower: one
        tower pass over all of them; else the tower once per utterance."""
        from . import check, lib
        from .ops import Tensor
        if not 1 <= len(samples_list) <= MAX_GROUP:
            raise OmxError(f"funasr-nano: {len(samples_list)} utterances in one group (1..{MAX_GROUP})")
        feats = [self.lfr_rows(s) for s in samples_list]
        lengths = [f.shape[0] for f in feats]
        if not self.joint_tower or len(feats) == 1:
            return [self.encoder.forward(f, [n]) for f, n in zip(feats, lengths)]
        width = feats[0].shape[1]
        stacked = Tensor((sum(lengths), width), "f32")
        at = 0
        for f, n in zip(feats, lengths):
            check(lib.omx_memcpy_d2d(stacked.ptr + at * width * 4, f.ptr, n * width * 4, None))
            at += n
        out = self.encoder.forward(stacked, lengths)
        d = out.shape[1]
        offs = np.concatenate([[0], np.cumsum(lengths)])
        return [out.slice_rows(int(offs[u]) * d, (lengths[u], d)) for u in range(len(lengths))]

    # ---- rows -> tokens ----

    def _set_sampler(self, target, cfg: SamplingConfig, *slot):
        target.set_sampler(*slot, float(cfg.temperature), int(cfg.seed), top_k=int(cfg.top_k), top_p=float(cfg.top_p),
                           repetition_penalty=float(cfg.repetition_penalty))

    def generate_ids(self, rows, config: Optional[SamplingConfig] = None, prompt: Optional[Prompt] = None) -> List[int]:
        """generate_text_with_config (model.rs:532-663) up to the token ids, on engine.Model"""
        cfg = config or SamplingConfig()
        ids, at = (prompt or self.prompt).ids(rows.shape[0])
        self.model.reset()
        self._set_sampler(self.model, cfg)
        first = self.model.prefill(ids, embeds=rows, embeds_at=at)
        return generate_ids(self.model, first, StopRule(self.markers, cfg.max_tokens))

    def _batch(self, n_slots: int):
        if n_slots not in self._batches:
            self._batches[n_slots] = self.model.batch(n_slots, 0, kv_bits=self.kv_bits)
        return self._batches[n_slots]

    def generate_ids_batch(self, rows_list, config: Optional[SamplingConfig] = None, prompt: Optional[Prompt] = None) -> List[List[int]]:
        """up to 8 utterances' rows through one Batch: a prompt pass per slot, then decode steps over the slots still running"""
        cfg = config or SamplingConfig()
        self.model.set_sampler(0.0)          # (a batch's prompt pass refuses a model whose own sampler has filters on)
        b = self._batch(len(rows_list))
        firsts = []
        for slot, rows in enumerate(rows_list):
            ids, at = (prompt or self.prompt).ids(rows.shape[0])
            b.reset(slot)
            self._set_sampler(b, cfg, slot)
            firsts.append(b.prefill(slot, ids, embeds=rows, embeds_at=at))
        return generate_ids_batch(b, firsts, [StopRule(self.markers, cfg.max_tokens) for _ in rows_list])

    def transcribe_ids_batch(self, samples_list, config: Optional[SamplingConfig] = None, prompt: Optional[Prompt] = None) -> List[List[int]]:
        """any number of 16 kHz utterances, in groups of up to 8: one tower pass and one Batch per group"""
        out: List[List[int]] = []
        for g in groups(len(samples_list)):
            rows = self.encode_audio([samples_list[i] for i in g])
            out.extend(self.generate_ids_batch(rows, config, prompt))
        return out

    # ---- the reference's entry points ----

    def _to_16k(self, samples, rate: int) -> np.ndarray:
        from . import audio
        s = np.asarray(samples, dtype=np.float32)
        return audio.resample(s, int(rate), self.frontend.sample_rate) if int(rate) != self.frontend.sample_rate else s

    def _text(self, ids: List[int]) -> str:
        return self.tokenizer.decode(ids, skip_special_tokens=True)

    def transcribe_samples(self, samples, rate: int = 16000, config: Optional[SamplingConfig] = None, prompt: Optional[Prompt] = None) -> str:
        rows = self.encode_audio([self._to_16k(samples, rate)])[0]
        return self._text(self.generate_ids(rows, config, prompt))

    def transcribe(self, path: str, config: Optional[SamplingConfig] = None) -> str:
        from . import audio
        samples, rate = audio.load_wav(path)
        return self.transcribe_samples(samples, rate, config)

    def transcribe_with_prompt(self, path: str, system: str, instruction: str, config: Optional[SamplingConfig] = None) -> str:
        from . import audio
        samples, rate = audio.load_wav(path)
        return self.transcribe_samples(samples, rate, config, build_prompt(self.tokenizer, self.markers, system, instruction))

    def transcribe_samples_batch(self, samples_list, config: Optional[SamplingConfig] = None) -> List[str]:
        """[(samples, rate), ...] -> texts, in order (model.rs:455-476, batched here)"""
        clips = [self._to_16k(s, r) for s, r in samples_list]
        return [self._text(ids) for ids in self.transcribe_ids_batch(clips, config)]
