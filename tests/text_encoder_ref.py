"""float64 restatement of the sentence encoder (HF BertModel, post-LN, + sentence-transformers Pooling / Normalize) for the
text-encoder tests: numpy only (erf from scipy), so that a GPU test needs neither a HF model run nor anything outside the tree.
The `wrong` switches build the mistaken variants whose distance from the right arithmetic the test docstrings quote."""
import os
import shutil

import numpy as np
from scipy.special import erf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TINY = os.path.join(GOLD, "tiny_minilm")


def ln(x, g, b, eps):
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + eps) * g + b


def gelu(x, tanh=False):
    if tanh:
        return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def attention(q, k, v, H):
    """full softmax self-attention of one sequence: q, k, v float64 [n, H * dh]"""
    n, D = q.shape
    dh = D // H
    out = np.empty_like(q)
    for h in range(H):
        c = slice(h * dh, (h + 1) * dh)
        s = q[:, c] @ k[:, c].T * dh ** -0.5
        s = np.exp(s - s.max(-1, keepdims=True))
        out[:, c] = (s / s.sum(-1, keepdims=True)) @ v[:, c]
    return out


def pool(x, mode, normalize):
    if mode == "mean":
        e = x.sum(0) / max(float(x.shape[0]), 1e-9)
    elif mode == "cls":
        e = x[0].copy()
    else:
        e = x.max(0)
    if normalize:
        e = e / max(float(np.sqrt((e * e).sum())), 1e-12)
    return e


def encode_ref(W, cfg, ids, pooling="mean", normalize=True, hidden=None, wrong=()):
    """W {HF name: array}, cfg the config.json dict, ids a list of token id lists -> float64 [n, D]; `hidden` (a list) receives, per
    sentence, the [len, D] states after the embedding and after every layer.
    wrong: any of "tanh_gelu", "eps1e-5", "no_specials" (mean over the inner tokens), "cls", "no_type"."""
    W = {k: np.asarray(v, np.float64) for k, v in W.items()}
    H, eps = cfg["num_attention_heads"], (1e-5 if "eps1e-5" in wrong else cfg["layer_norm_eps"])
    e = "embeddings."
    out = []
    for s in ids:
        s = np.asarray(s, np.int64)
        x = W[e + "word_embeddings.weight"][s] + W[e + "position_embeddings.weight"][np.arange(len(s))]
        if "no_type" not in wrong:
            x = x + W[e + "token_type_embeddings.weight"][0]
        x = ln(x, W[e + "LayerNorm.weight"], W[e + "LayerNorm.bias"], eps)
        states = [x]
        for i in range(cfg["num_hidden_layers"]):
            p = "encoder.layer.%d." % i
            a = p + "attention.self."
            q, k, v = (x @ W[a + n + ".weight"].T + W[a + n + ".bias"] for n in ("query", "key", "value"))
            y = attention(q, k, v, H) @ W[p + "attention.output.dense.weight"].T + W[p + "attention.output.dense.bias"] + x
            x = ln(y, W[p + "attention.output.LayerNorm.weight"], W[p + "attention.output.LayerNorm.bias"], eps)
            h = gelu(x @ W[p + "intermediate.dense.weight"].T + W[p + "intermediate.dense.bias"], "tanh_gelu" in wrong)
            y = h @ W[p + "output.dense.weight"].T + W[p + "output.dense.bias"] + x
            x = ln(y, W[p + "output.LayerNorm.weight"], W[p + "output.LayerNorm.bias"], eps)
            states.append(x)
        if hidden is not None:
            hidden.append(states)
        xp = x[1:-1] if ("no_specials" in wrong and len(s) > 2) else x
        out.append(pool(xp, "cls" if "cls" in wrong else pooling, normalize))
    return np.stack(out)


def rel_err(a, b):
    """max |a - b| relative to max |b| (the README's bar: relative to the tensor's scale)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def load_tiny_weights(model_dir=TINY):
    from safetensors.numpy import load_file
    return load_file(os.path.join(model_dir, "model.safetensors"))


def cls_variant_dir(tmp_path, model_dir=TINY):
    """a copy of the fixture whose modules.json is the committed sibling variant (cls pooling, no Normalize)"""
    dst = os.path.join(str(tmp_path), "tiny_minilm_cls")
    shutil.copytree(model_dir, dst)
    shutil.copyfile(os.path.join(dst, "modules_cls.json"), os.path.join(dst, "modules.json"))
    return dst


def plain_hf_dir(tmp_path, model_dir=TINY):
    """a copy of the fixture as a plain HF BertModel directory: no sentence-transformers files, keys with a `bert.` prefix"""
    import json
    from safetensors.numpy import load_file, save_file
    dst = os.path.join(str(tmp_path), "tiny_bert_plain")
    os.makedirs(dst)
    for f in ("config.json", "tokenizer.json", "tokenizer_config.json", "vocab.txt", "special_tokens_map.json"):
        if os.path.exists(os.path.join(model_dir, f)):
            shutil.copyfile(os.path.join(model_dir, f), os.path.join(dst, f))
    W = load_file(os.path.join(model_dir, "model.safetensors"))
    W = {"bert." + k: v for k, v in W.items()}
    D = json.load(open(os.path.join(dst, "config.json")))["hidden_size"]
    W["bert.pooler.dense.weight"], W["bert.pooler.dense.bias"] = np.zeros((D, D), np.float32), np.zeros((D,), np.float32)
    W["bert.embeddings.position_ids"] = np.arange(4, dtype=np.int64)[None]
    save_file(W, os.path.join(dst, "model.safetensors"))
    return dst


def train_records(raw):
    """evqa8 raw records in the training-record layout build_ike_corpus reads"""
    return [{"prompt": r["src"], "target": r["alt"], "rephrase_prompt": r["rephrase"], "locality_prompt": r["loc"],
             "locality_ground_truth": r["loc_ans"], "image_path": r["image"], "rephrase_image_path": r["image_rephrase"],
             "locality_image_path": r["m_loc"]} for r in raw]
