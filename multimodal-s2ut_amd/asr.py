"""ASR transcription of synthesized speech: HF ``Wav2Vec2ForCTC`` (the wav2vec2-large family with
feat_extract_norm "layer" and do_stable_layer_norm) forward on HIP kernels, then greedy CTC decoding --
the step of the reference pipeline between the vocoder and BLEU (mm_s2ut/scripts/transcript.py).

Forward only.  The feature extractor and the positional convolution run one utterance at a time on the
kernels of csrc/asr.hip (no padding ever enters a convolution); the transformer layers run on the GEMM,
LayerNorm and flash-attention kernels of the training path, on up to ``batch_size`` utterances packed
as [B, Tmax, d] with key-length masking.  Activations are time-major fp16 [T, C]; the logits are fp32.
Weight norm is folded and the weights are repacked into the kernels' layouts once, at load.  The loaders,
the layer loop and the packing are encoders.py's (SpeechEncoder, shared with units.py); what is here is
the layer-norm feature extractor, the CTC head and the decoding.

``transformers`` is not a dependency: the semantics are restated here (and in tests/asr_ref.py), the
checkpoint's key names and tensor layouts pin the loader."""
import os

import torch

from . import kernels as K
from .encoders import (CONFIG_DEFAULTS, CONV_LN_EPS, NORM_EPS, SAMPLE_RATE, SpeechEncoder, Weights,
                       fold_pos_conv_weight_norm, load_state_dict, read_json, validate_config, wave_batches)
# re-exported: part of this module's surface
from .encoders import (frame_counts as frame_counts, read_safetensors as read_safetensors, read_wav as read_wav,
                       receptive_field as receptive_field)

CLEANUP = ((" .", "."), (" ?", "?"), (" !", "!"), (" ,", ","), (" ' ", "'"), (" n't", "n't"), (" 'm", "'m"),
           (" 's", "'s"), (" 've", "'ve"), (" 're", "'re"))


class NonFiniteLogits(RuntimeError):
    """An utterance's logits hold inf or NaN (fp16 activations overflowed): no transcript is written."""


def parse_config(cfg):
    """Validated copy of a Wav2Vec2 config.json dict (the keys the forward reads)."""
    return validate_config(cfg, "wav2vec2", CONFIG_DEFAULTS, "layer", True, False)


def collapse(ids, blank):
    """Frame ids -> CTC token ids: runs of equal ids collapse to one, then the blank drops."""
    out, prev = [], None
    for i in ids:
        i = int(i)
        if i != prev and i != blank:
            out.append(i)
        prev = i
    return out


def tokens_to_text(tokens, id_to_token, delimiter="|", cleanup=True, lower=False):
    """Collapsed token ids -> text as Wav2Vec2CTCTokenizer decodes them: the word delimiter becomes a
    space, the string is stripped (and lower-cased with do_lower_case), and with cleanup HF's fixed list
    of replacements applies."""
    s = "".join(" " if id_to_token[t] == delimiter else id_to_token[t] for t in tokens).strip()
    if lower:
        s = s.lower()
    if cleanup:
        for a, b in CLEANUP:
            s = s.replace(a, b)
    return s


def greedy_decode(ids, id_to_token, blank, delimiter="|", cleanup=True, lower=False):
    """Per-frame argmax ids -> text (host restatement of the device path: collapse + tokens_to_text)."""
    return tokens_to_text(collapse(ids, blank), id_to_token, delimiter, cleanup, lower)


class Wav2Vec2CTC(SpeechEncoder):
    """HF Wav2Vec2ForCTC in eval mode plus Wav2Vec2Processor's normalisation and greedy decoding."""

    def __init__(self, state_dict, config, vocab, tokenizer_cfg=None, preprocessor_cfg=None, device="cuda"):
        c = parse_config(config)
        tok, pre = dict(tokenizer_cfg or {}), dict(preprocessor_cfg or {})
        self.delimiter = tok.get("word_delimiter_token", "|")
        self.cleanup = bool(tok.get("clean_up_tokenization_spaces", True))
        self.lower = bool(tok.get("do_lower_case", False))
        if not pre.get("do_normalize", True):
            raise NotImplementedError("preprocessor_config.json with do_normalize false is not supported (the "
                                      "layer-norm wav2vec2 models normalise each utterance)")
        self.blank = int(c["pad_token_id"])
        self.V = V = int(c["vocab_size"])
        self.id_to_token = {int(i): t for t, i in vocab.items()}
        if sorted(self.id_to_token) != list(range(V)):
            raise ValueError(f"vocab.json (with added_tokens.json, where the directory has one) does not map onto "
                             f"the ids 0..{V - 1} of the head (vocab_size {V})")
        if not 0 <= self.blank < V:
            raise ValueError(f"pad_token_id {self.blank} outside the vocabulary of {V}")
        w = Weights(fold_pos_conv_weight_norm(state_dict), "wav2vec2 checkpoint", device)
        super().__init__(w, c, "wav2vec2.", c["num_hidden_layers"], pre.get("sampling_rate", SAMPLE_RATE))
        self.Vp = K.round_up(V, 8)
        hw = torch.zeros(self.Vp, self.d)
        hw[:V] = w.get("lm_head.weight", (V, self.d))
        self.head_w, self.head_b = w.f16(hw), w.f32(w.get("lm_head.bias", (V,)))

    @classmethod
    def from_pretrained(cls, model_dir, device="cuda"):
        vocab = dict(read_json(model_dir, "vocab.json", True))
        vocab.update(read_json(model_dir, "added_tokens.json") or {})      # tokens the tokenizer keeps outside vocab.json
        return cls(load_state_dict(model_dir), read_json(model_dir, "config.json", True), vocab,
                   read_json(model_dir, "tokenizer_config.json"), read_json(model_dir, "preprocessor_config.json"), device)

    # ---------------------------------------------------------------------------------- forward

    def extract(self, x):
        """fp32 waveform on the device -> fp16 [T, d]: the feature extractor and the feature projection."""
        stats = K.wave_stats(x, NORM_EPS)
        c0 = self.conv[0]
        h = K.asr_conv0(x, stats, c0.w, c0.b, c0.g, c0.be, c0.stride, CONV_LN_EPS)
        for c in self.conv[1:]:
            h = K.asr_conv(h, c.w, c.b, c.cout, c.k, c.stride)
            K.asr_ln_gelu(h, c.g, c.be, CONV_LN_EPS)
        y = K.layernorm(h, self.fp_g, self.fp_b, self.eps)[0]
        return K.linear(y, self.fp_w, self.fp_bias)

    def encode(self, Hb, lens32=None):
        """fp16 [B, Tmax, d] (rows past an utterance's length: anything finite) -> fp32 [B, Tmax, Vp]: the
        stable-LN layers, encoder.layer_norm and the head without its bias (ctc_greedy adds it)."""
        return self.head(self.layers_forward(Hb, lens32), Hb.shape[0], Hb.shape[1])

    def head(self, X, B, Tm):
        """encoder.layer_norm and lm_head (bias left to ctc_greedy): fp16 [B * Tmax, d] -> fp32 [B, Tmax, Vp]."""
        y = K.layernorm(X, self.enc_g, self.enc_b, self.eps)[0]
        logits = torch.empty(B, Tm, self.Vp, dtype=torch.float32, device=X.device)
        K.gemm(y, self.head_w, logits, B * Tm, self.Vp, self.d, lda=self.d, ldb=self.d, ldc=self.Vp, epi=K.EPI_F32)
        return logits

    def forward_batch(self, waves, sr=None):
        """Waveforms -> (logits fp32 [B, Tmax, Vp] with the head's bias, lens (list), ids, out, count, bad:
        kernels.ctc_greedy's results), all on the device."""
        Hb, lens, lens32 = self.pack(waves, sr)
        logits = self.encode(Hb, lens32)
        return (logits, lens) + K.ctc_greedy(logits, self.V, self.blank, lens32, self.head_b)

    def _texts(self, lens, out, count, bad, cleanup):
        cleanup = self.cleanup if cleanup is None else cleanup
        count, bad, out = count.tolist(), bad.tolist(), out.cpu()
        for b, flag in enumerate(bad):
            if flag:
                raise NonFiniteLogits(f"utterance {b} of the batch ({lens[b]} frames): non-finite logits (the fp16 "
                                      "activations overflowed); no transcript written")
        return [tokens_to_text(out[b, :count[b]].tolist(), self.id_to_token, self.delimiter, cleanup, self.lower)
                for b in range(len(lens))]

    def logits(self, wave, sr=None):
        """fp32 [T, V] logits of one utterance (on the device)."""
        logits, lens, _, _, _, bad = self.forward_batch([wave], sr)
        if int(bad[0]):
            raise NonFiniteLogits(f"non-finite logits ({lens[0]} frames): the fp16 activations overflowed")
        return logits[0, :lens[0], :self.V]

    def transcribe(self, wave, sr=None, cleanup=None):
        return self.transcribe_many([wave], 1, sr, cleanup)[0]

    def transcribe_many(self, waves, batch_size=8, sr=None, cleanup=None):
        """Transcripts of the waveforms, in order; the encoder runs on batch_size utterances at a time."""
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        waves, texts = list(waves), []
        for i in range(0, len(waves), batch_size):
            _, lens, _, out, count, bad = self.forward_batch(waves[i:i + batch_size], sr)
            texts += self._texts(lens, out, count, bad, cleanup)
        return texts


def wav_sort_key(name):
    """The reference's order of {i}_pred.wav files: by the integer before the first '_'."""
    try:
        return int(name.split("_")[0])
    except ValueError:
        raise ValueError(f"'{name}': file names must start with an integer and '_' ({{i}}_pred.wav); the "
                         "directory must hold nothing but the synthesized WAV files") from None


def transcribe_dir(model, wav_dir, transcript_txt, batch_size=8):
    """Transcribe every file of wav_dir in the reference's order; transcripts joined by newlines with
    no trailing newline, as the reference writes them.  -> the number of files."""
    files = sorted(os.listdir(wav_dir), key=wav_sort_key)
    texts = []
    for _, waves in wave_batches(wav_dir, files, batch_size, model.sampling_rate):
        texts += model.transcribe_many(waves, batch_size)
    with open(transcript_txt, "w") as f:
        f.write("\n".join(texts))
    return len(files)
