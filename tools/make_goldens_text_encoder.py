"""Writes the sentence-encoder fixture and its goldens (CPU only; transformers.BertModel in float64 and the `tokenizers` library):

  tests/golden/tiny_minilm/            a sentence-transformers directory (modules.json, sentence_bert_config.json, 1_Pooling, Normalize):
                                       hidden 48, 3 heads (dh 16), FFN 96, 2 layers, 128 positions, max_seq_length 96; a lower-casing
                                       WordPiece tokenizer over the words of tests/golden/evqa8_records.json plus single characters and
                                       their ## forms; weights from synth.bert_param_init (std 0.1); and the sibling pooling variant
                                       modules_cls.json + 1_Pooling_cls (cls pooling, no Normalize)
  tests/golden/tiny_text_goldens.json  the sentences, their token ids, the retrieval corpus' rank gaps
  tests/golden/tiny_text_goldens.npz   float64 embeddings under both pooling configs, the per-layer hidden states of sentence 0, the
                                       embeddings of the 24 IKE corpus sentences

    python tools/make_goldens_text_encoder.py
"""
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLD, "tiny_minilm")

CFG = {"architectures": ["BertModel"], "model_type": "bert", "hidden_size": 48, "num_attention_heads": 3, "intermediate_size": 96,
       "num_hidden_layers": 2, "max_position_embeddings": 128, "type_vocab_size": 2, "hidden_act": "gelu", "layer_norm_eps": 1e-12,
       "position_embedding_type": "absolute", "attention_probs_dropout_prob": 0.0, "hidden_dropout_prob": 0.0, "pad_token_id": 0,
       "initializer_range": 0.1}
MAX_SEQ = 96
SEED = 20251121
SHORT = ["pans", "tennis balls", "how many pans do you see"]


def _dump(path, obj):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(obj, f, indent=1)
        f.write("\n")


def build_tokenizer(records):
    from tokenizers import Tokenizer, decoders, models, normalizers, pre_tokenizers, processors
    text = json.dumps(records).lower()
    words = sorted(set(re.findall(r"[a-z0-9]+", text)))
    chars = [chr(c) for c in range(33, 127) if not chr(c).isupper()]
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + chars + ["##" + c for c in chars if c.isalnum()]
    vocab += [w for w in words if w not in set(vocab)]
    vmap = {t: i for i, t in enumerate(vocab)}
    tok = Tokenizer(models.WordPiece(vmap, unk_token="[UNK]", max_input_chars_per_word=100))
    tok.normalizer = normalizers.BertNormalizer(lowercase=True)
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    tok.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1",
                                                       special_tokens=[("[CLS]", vmap["[CLS]"]), ("[SEP]", vmap["[SEP]"])])
    tok.decoder = decoders.WordPiece(prefix="##")
    os.makedirs(OUT, exist_ok=True)
    tok.save(os.path.join(OUT, "tokenizer.json"))
    with open(os.path.join(OUT, "vocab.txt"), "w") as f:
        f.write("\n".join(vocab) + "\n")
    _dump(os.path.join(OUT, "tokenizer_config.json"),
          {"tokenizer_class": "BertTokenizer", "do_lower_case": True, "model_max_length": CFG["max_position_embeddings"],
           "unk_token": "[UNK]", "sep_token": "[SEP]", "pad_token": "[PAD]", "cls_token": "[CLS]", "mask_token": "[MASK]"})
    _dump(os.path.join(OUT, "special_tokens_map.json"),
          {"unk_token": "[UNK]", "sep_token": "[SEP]", "pad_token": "[PAD]", "cls_token": "[CLS]", "mask_token": "[MASK]"})
    return len(vocab)


def hf_embed(model, ids, pooling, normalize, hidden=None):
    """transformers.BertModel (float64), one sentence per call (no padding), + sentence-transformers' pooling arithmetic"""
    out = []
    for s in ids:
        with torch.no_grad():
            o = model(input_ids=torch.tensor([s]), output_hidden_states=True)
        h = o.last_hidden_state[0]
        if hidden is not None:
            hidden.append([t[0].numpy() for t in o.hidden_states])
        if pooling == "mean":
            e = h.sum(0) / max(float(h.shape[0]), 1e-9)
        elif pooling == "cls":
            e = h[0]
        else:
            e = h.max(0).values
        if normalize:
            e = e / e.norm().clamp_min(1e-12)
        out.append(e.numpy())
    return np.stack(out)


def main():
    from safetensors.numpy import save_file
    from transformers import AutoTokenizer, BertConfig, BertModel
    from devqa_amd.synth import bert_param_init, bert_param_shapes
    from devqa_amd.editor.vllm_editors.ike_vl.ike_vl import build_ike_corpus, ike_sentence
    import text_encoder_ref as T

    rec = json.load(open(os.path.join(GOLD, "evqa8_records.json")))
    cfg = dict(CFG, vocab_size=build_tokenizer(rec))
    _dump(os.path.join(OUT, "config.json"), cfg)
    _dump(os.path.join(OUT, "sentence_bert_config.json"), {"max_seq_length": MAX_SEQ, "do_lower_case": False})
    _dump(os.path.join(OUT, "modules.json"),
          [{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
           {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
           {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}])
    _dump(os.path.join(OUT, "modules_cls.json"),
          [{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
           {"idx": 1, "name": "1", "path": "1_Pooling_cls", "type": "sentence_transformers.models.Pooling"}])
    pool = {"word_embedding_dimension": cfg["hidden_size"], "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True,
            "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False}
    _dump(os.path.join(OUT, "1_Pooling", "config.json"), pool)
    _dump(os.path.join(OUT, "1_Pooling_cls", "config.json"), dict(pool, pooling_mode_cls_token=True, pooling_mode_mean_tokens=False))
    W = {n: bert_param_init(n, s, SEED) for n, s in bert_param_shapes(cfg).items()}
    save_file(W, os.path.join(OUT, "model.safetensors"))

    # ---- sentences ----
    queries = []
    for r in rec["records"]:
        q = r["requests"][0]
        nf = q["prompt"] + " " + q["target_new"]
        queries.append(ike_sentence(nf, nf))
    long_s = " ".join(r["locality"]["text_loc"][0]["prompt"] + " " + r["locality"]["text_loc"][0]["target"] for r in rec["records"])
    sentences = queries + SHORT + [long_s]
    tok = AutoTokenizer.from_pretrained(OUT)
    enc = lambda ss: tok(ss, add_special_tokens=True, truncation=True, max_length=MAX_SEQ, padding=False)["input_ids"]
    ids = enc(sentences)
    full_long = tok([long_s], add_special_tokens=True, truncation=False)["input_ids"][0]
    assert len(full_long) > MAX_SEQ and len(ids[-1]) == MAX_SEQ, (len(full_long), len(ids[-1]))
    print("token counts:", [len(s) for s in ids], "untruncated long:", len(full_long))

    # ---- float64 HF model ----
    model = BertModel(BertConfig(**cfg), add_pooling_layer=False).double().eval()
    missing = model.load_state_dict({k: torch.from_numpy(v).double() for k, v in W.items()}, strict=False)
    assert not missing.unexpected_keys and all("position_ids" in k for k in missing.missing_keys), missing
    hid = []
    e_mean = hf_embed(model, ids, "mean", True, hid)
    e_cls = hf_embed(model, ids, "cls", False)
    # the numpy restatement the tests use must say the same
    assert np.abs(T.encode_ref(W, cfg, ids, "mean", True) - e_mean).max() < 1e-12
    assert np.abs(T.encode_ref(W, cfg, ids, "cls", False) - e_cls).max() < 1e-12

    # ---- how far the wrong variants lie (quoted in the test docstrings) ----
    scale = np.abs(e_mean).max()
    for wv in ("tanh_gelu", "eps1e-5", "no_specials", "cls", "no_type"):
        print("wrong variant %-12s max-abs distance / scale = %.2e" % (wv, np.abs(T.encode_ref(W, cfg, ids, "mean", True, wrong=(wv,)) - e_mean).max() / scale))

    # ---- retrieval: 24 corpus sentences (3 per training record), the 8 queries, k = 3 ----
    train = T.train_records(rec["raw"])
    corpus = build_ike_corpus(train, lambda ss: T.encode_ref(W, cfg, enc(ss), "mean", True))
    c_emb = T.encode_ref(W, cfg, enc(corpus["sentences"]), "mean", True)
    sims = e_mean[:8] @ c_emb.T                                   # both sides are unit vectors
    order = np.argsort(-sims, 1, kind="stable")
    srt = np.take_along_axis(sims, order, 1)
    gaps = srt[:, 2] - srt[:, 3]
    print("rank 3/4 gaps:", gaps, " rank 1/2 gaps:", srt[:, 0] - srt[:, 1])
    assert (gaps > 1e-4).sum() >= 7, "pick other sentences: more than one query has a rank-3/4 near-tie"

    _dump(os.path.join(GOLD, "tiny_text_goldens.json"),
          {"sentences": sentences, "ids": ids, "n_queries": 8, "long_untruncated_tokens": len(full_long), "max_seq_length": MAX_SEQ,
           "top3": order[:, :3].tolist(), "gap34": gaps.tolist(), "seed": SEED})
    np.savez(os.path.join(GOLD, "tiny_text_goldens.npz"), emb_mean_norm=e_mean, emb_cls=e_cls, corpus_emb=c_emb,
             top3_scores=srt[:, :3], **{"hidden0_%d" % i: h for i, h in enumerate(hid[0])})
    print("wrote", OUT, "and tiny_text_goldens.{json,npz}")


if __name__ == "__main__":
    main()
