"""Native sentence encoder: a BERT-family text tower (all-MiniLM-L6-v2 in the reference: R/dataset/vllm.py:66,91,
R/easyeditor/models/ike/ike_main.py:185-200) on the HIP path, with the pooling and normalisation modules of its
sentence-transformers directory.

`SentenceEncoder(model_dir).encode(sentences)` is the `encode` callable IKEvl, LTEvl, EmbeddingRetriever and build_ike_corpus
take; `.encode_device` leaves the embeddings on the device, fp32 contiguous [n, D], which is what lib.cosine_topk reads.

Arithmetic (HF BertModel, post-LN), per pass of packed token rows (no padding: one attention descriptor per sentence):
    x = LN((word[token] + type[0]) + position[pos])                              devqa_text_embed_ln
    per layer:  qkv = x Wqkv^T + b          (q | k | v fused into one GEMM)       devqa_gemm_*
                a   = softmax(q k^T dh^-0.5) v    (full self-attention)           devqa_attention*
                x   = LN(a Wo^T + bo + x)                                         devqa_gemm_* (residual), devqa_layernorm
                x   = LN(gelu(x W1^T + b1) W2^T + b2 + x)     (erf GELU)          devqa_gemm_* (GELU / residual), devqa_layernorm
    e = pool(x) [/ max(||.||, 1e-12)]                                            devqa_seq_pool
dtype "bf16": bf16 weights and GEMM operands, fp32 accumulation, fp32 residual stream and LayerNorm; "fp32" (faithful mode):
fp32 weights and the exact-fp32 GEMM / attention kernels.  There is no torch fallback: every FLOP above is a library call.

Supported: `model_type == "bert"`, absolute positions, `hidden_act == "gelu"`.  MPNet (relative-position attention bias; LTE_VL's
multi-qa-mpnet-base-dot-v1) is not: it raises NotImplementedError."""
import json
import os
from typing import List, Sequence

import numpy as np
import torch

from . import lib

POOL_MODES = {"mean": lib.POOL_MEAN, "cls": lib.POOL_CLS, "max": lib.POOL_MAX}


def _read_json(path):
    with open(path, "r") as f:
        return json.load(f)


def is_bert_dir(path) -> bool:
    """True for an existing directory whose config.json says model_type "bert" (what SentenceEncoder can load)."""
    cfg = os.path.join(str(path), "config.json") if path else None
    if not cfg or not os.path.isfile(cfg):
        return False
    try:
        return _read_json(cfg).get("model_type") == "bert"
    except (OSError, ValueError):
        return False


def mode_of(vllm) -> str:
    """the compute mode of a model wrapper ("fp32" for the faithful wrapper, else "bf16"): the mode an editor's encoder is built in"""
    return "fp32" if getattr(getattr(vllm, "engine", None), "adt", None) == torch.float32 else "bf16"


def read_model_layout(model_dir):
    """-> (config dict, max_seq_length, pooling name, normalize) of a sentence-transformers directory (modules.json) or of a
    plain HF BertModel directory (mean pooling, no normalisation, max_seq_length = max_position_embeddings)."""
    cfg_path = os.path.join(model_dir, "config.json")
    if not os.path.isfile(cfg_path):
        raise FileNotFoundError("no config.json in %s" % model_dir)
    cfg = _read_json(cfg_path)
    if cfg.get("model_type") != "bert":
        raise NotImplementedError("SentenceEncoder: model_type %r is not supported (only \"bert\"; MPNet needs a relative-position "
                                  "attention bias)" % cfg.get("model_type"))
    if cfg.get("position_embedding_type", "absolute") != "absolute":
        raise NotImplementedError("SentenceEncoder: position_embedding_type %r is not supported (only \"absolute\")"
                                  % cfg["position_embedding_type"])
    if cfg.get("hidden_act", "gelu") != "gelu":
        raise NotImplementedError("SentenceEncoder: hidden_act %r is not supported (only \"gelu\")" % cfg["hidden_act"])
    if cfg["hidden_size"] % cfg["num_attention_heads"] or cfg["hidden_size"] % 4:
        raise NotImplementedError("SentenceEncoder: hidden_size %d with %d heads is not supported"
                                  % (cfg["hidden_size"], cfg["num_attention_heads"]))
    max_len, pooling, normalize = int(cfg["max_position_embeddings"]), "mean", False
    mod_path = os.path.join(model_dir, "modules.json")
    if os.path.isfile(mod_path):
        for m in _read_json(mod_path):
            kind, sub = m["type"].rsplit(".", 1)[-1], os.path.join(model_dir, m.get("path", ""))
            if kind == "Transformer":
                sb = os.path.join(sub, "sentence_bert_config.json")
                if os.path.isfile(sb):
                    msl = _read_json(sb).get("max_seq_length")
                    if msl is not None:
                        max_len = min(max_len, int(msl))
            elif kind == "Pooling":
                pc = _read_json(os.path.join(sub, "config.json"))
                on = [k for k, v in pc.items() if k.startswith("pooling_mode_") and v is True]
                names = {"pooling_mode_mean_tokens": "mean", "pooling_mode_cls_token": "cls", "pooling_mode_max_tokens": "max"}
                if len(on) != 1 or on[0] not in names:
                    raise NotImplementedError("SentenceEncoder: pooling %s is not supported (exactly one of mean / cls / max)" % on)
                pooling = names[on[0]]
            elif kind == "Normalize":
                normalize = True
            else:
                raise NotImplementedError("SentenceEncoder: sentence-transformers module %r is not supported" % m["type"])
    return cfg, max_len, pooling, normalize


def load_bert_state(model_dir):
    """{name: torch tensor} of model.safetensors or pytorch_model.bin, keys without a `bert.` prefix, pooler and position_ids
    dropped."""
    st_path, bin_path = os.path.join(model_dir, "model.safetensors"), os.path.join(model_dir, "pytorch_model.bin")
    if os.path.isfile(st_path):
        from safetensors.torch import load_file
        sd = load_file(st_path)
    elif os.path.isfile(bin_path):
        sd = torch.load(bin_path, map_location="cpu", weights_only=True)
    else:
        raise FileNotFoundError("no model.safetensors or pytorch_model.bin in %s" % model_dir)
    out = {}
    for k, v in sd.items():
        k = k[5:] if k.startswith("bert.") else k
        if k.startswith("pooler.") or k.endswith("position_ids"):
            continue
        out[k] = v
    return out


class SentenceEncoder:
    def __init__(self, model_dir, device="cuda:0", dtype="bf16", max_rows=32768):
        if dtype not in ("bf16", "fp32"):
            raise ValueError("dtype must be 'bf16' or 'fp32'")
        model_dir = str(model_dir)
        self.cfg, self.max_seq_length, self.pooling, self.normalize = read_model_layout(model_dir)
        sd = load_bert_state(model_dir)
        from transformers import AutoTokenizer
        self.tokenizer = AutoTokenizer.from_pretrained(model_dir)
        c = self.cfg
        self.device = torch.device(device)
        self.dtype = dtype
        self.wdt = torch.bfloat16 if dtype == "bf16" else torch.float32
        self.dim = self.D = int(c["hidden_size"])
        self.H = int(c["num_attention_heads"])
        self.dh = self.D // self.H
        self.n_layers = int(c["num_hidden_layers"])
        self.eps = float(c.get("layer_norm_eps", 1e-12))
        self.max_rows = max(int(max_rows), self.max_seq_length)    # a pass holds at least one whole sentence

        def take(name):
            if name not in sd:
                raise KeyError("SentenceEncoder: %s has no weight %r" % (model_dir, name))
            return sd[name].to(torch.float32)

        def w(t):           # GEMM operand / table in the compute dtype
            return t.to(self.wdt).to(self.device).contiguous()

        def f(t):           # biases and LayerNorm parameters stay fp32 in both modes
            return t.to(self.device).contiguous()

        e = "embeddings."
        self.word, self.position = w(take(e + "word_embeddings.weight")), w(take(e + "position_embeddings.weight"))
        self.type0 = w(take(e + "token_type_embeddings.weight")[0])
        self.emb_g, self.emb_b = f(take(e + "LayerNorm.weight")), f(take(e + "LayerNorm.bias"))
        self.V, self.P = self.word.shape[0], self.position.shape[0]
        if self.word.shape[1] != self.D or self.position.shape[1] != self.D or self.max_seq_length > self.P:
            raise ValueError("SentenceEncoder: tables %s / %s do not fit hidden_size %d, max_seq_length %d"
                             % (tuple(self.word.shape), tuple(self.position.shape), self.D, self.max_seq_length))
        self.layers = []
        for i in range(self.n_layers):
            p = "encoder.layer.%d." % i
            a = p + "attention.self."
            self.layers.append(dict(
                wqkv=w(torch.cat([take(a + "query.weight"), take(a + "key.weight"), take(a + "value.weight")], 0)),
                bqkv=f(torch.cat([take(a + "query.bias"), take(a + "key.bias"), take(a + "value.bias")], 0)),
                wo=w(take(p + "attention.output.dense.weight")), bo=f(take(p + "attention.output.dense.bias")),
                g1=f(take(p + "attention.output.LayerNorm.weight")), b1=f(take(p + "attention.output.LayerNorm.bias")),
                wi=w(take(p + "intermediate.dense.weight")), bi=f(take(p + "intermediate.dense.bias")),
                wd=w(take(p + "output.dense.weight")), bd=f(take(p + "output.dense.bias")),
                g2=f(take(p + "output.LayerNorm.weight")), b2=f(take(p + "output.LayerNorm.bias"))))

    # ------------------------------------------------------------------------------------------
    def tokenize(self, sentences: Sequence[str]) -> List[List[int]]:
        """[CLS] ... [SEP] ids per sentence, truncated to max_seq_length with the specials included, no padding."""
        sentences = [str(s) for s in sentences]
        if not sentences:
            return []
        return self.tokenizer(sentences, add_special_tokens=True, truncation=True, max_length=self.max_seq_length, padding=False,
                              return_attention_mask=False, return_token_type_ids=False)["input_ids"]

    def _check_ids(self, ids):
        """Host check before any launch: every token id inside the word table, every sentence inside the position table."""
        for s in ids:
            if len(s) == 0:
                raise ValueError("SentenceEncoder: an empty token sequence")
            if len(s) > self.max_seq_length:
                raise ValueError("SentenceEncoder: %d tokens exceed max_seq_length %d" % (len(s), self.max_seq_length))
            lo, hi = min(s), max(s)
            if lo < 0 or hi >= self.V:
                raise ValueError("SentenceEncoder: token id %d outside the word table [0, %d)" % (lo if lo < 0 else hi, self.V))

    def _passes(self, ids):
        """index ranges [i0, i1) of consecutive sentences whose token rows fit max_rows"""
        out, i0, rows = [], 0, 0
        for i, s in enumerate(ids):
            if rows and rows + len(s) > self.max_rows:
                out.append((i0, i))
                i0, rows = i, 0
            rows += len(s)
        if i0 < len(ids):
            out.append((i0, len(ids)))
        return out

    def _forward(self, ids, hidden=None):
        """one pass: packed rows of `ids` -> fp32 [len(ids), D] on the device; `hidden` (a list) receives the fp32 residual stream after
        the embedding and after every layer"""
        dev, D, H, dh = self.device, self.D, self.H, self.dh
        lens = np.asarray([len(s) for s in ids], np.int32)
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
        tok = np.concatenate([np.asarray(s, np.int32) for s in ids])
        pos = np.concatenate([np.arange(n, dtype=np.int32) for n in lens])
        zeros = np.zeros_like(lens)
        desc = np.stack([starts, lens, zeros, zeros, starts, lens], 1)
        meta = lib.h2d(torch.from_numpy(np.concatenate([tok, pos, starts, lens, desc.reshape(-1)])), torch.int32, dev)
        R, S = tok.size, lens.size
        tok_d, pos_d, st_d, ln_d = meta[:R], meta[R:2 * R], meta[2 * R:2 * R + S], meta[2 * R + S:2 * R + 2 * S]
        desc_d = meta[2 * R + 2 * S:].view(S, 6)
        max_len, scale = int(lens.max()), dh ** -0.5
        bf = self.wdt == torch.bfloat16
        both = "both" if bf else "f32"
        x = lib.text_embed_ln(tok_d, pos_d, self.word, self.position, self.type0, self.emb_g, self.emb_b, self.eps, want=both)
        xo, x = x if bf else (x, x)             # xo: the GEMM operand (bf16 copy, or the fp32 stream itself)
        if hidden is not None:
            hidden.append(x.clone())
        for L in self.layers:
            qkv = lib.gemm(xo, L["wqkv"], L["bqkv"])
            att = lib.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], desc_d, S, max_len, H, dh, scale, 0, self_full=True)
            y = lib.gemm(att, L["wo"], L["bo"], residual=x, want="f32")
            x = lib.layernorm(y, L["g1"], L["b1"], self.eps, want=both)
            xo, x = x if bf else (x, x)
            h = lib.gemm(xo, L["wi"], L["bi"], act=lib.ACT_GELU)
            y = lib.gemm(h, L["wd"], L["bd"], residual=x, want="f32")
            x = lib.layernorm(y, L["g2"], L["b2"], self.eps, want=both)
            xo, x = x if bf else (x, x)
            if hidden is not None:
                hidden.append(x.clone())
        return lib.seq_pool(x, st_d, ln_d, POOL_MODES[self.pooling], self.normalize)

    # ------------------------------------------------------------------------------------------
    def encode_ids(self, ids: Sequence[Sequence[int]]) -> torch.Tensor:
        """token id lists (specials included) -> fp32 [n, D] on the device"""
        ids = [list(map(int, s)) for s in ids]
        self._check_ids(ids)
        out = torch.empty((len(ids), self.D), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            for i0, i1 in self._passes(ids):
                out[i0:i1] = self._forward(ids[i0:i1])
        return out

    def encode_device(self, sentences: Sequence[str]) -> torch.Tensor:
        """sentences -> fp32 contiguous [n, D] on the device (the layout of lib.cosine_topk's queries and corpus); no host round trip"""
        if isinstance(sentences, str):
            sentences = [sentences]
        return self.encode_ids(self.tokenize(sentences))

    def encode(self, sentences: Sequence[str]) -> np.ndarray:
        """sentences -> np.float32 [n, D]: the `encode` callable of IKEvl / LTEvl / EmbeddingRetriever / build_ike_corpus"""
        return self.encode_device(sentences).cpu().numpy()

    __call__ = encode

    def hidden_states(self, sentences: Sequence[str]) -> List[torch.Tensor]:
        """fp32 [rows, D] residual stream after the embedding and after each layer, rows packed in sentence order (one pass; for
        localising a parity failure)"""
        ids = self.tokenize(sentences)
        self._check_ids(ids)
        hidden = []
        with torch.cuda.device(self.device):
            self._forward(ids, hidden)
        return hidden
