"""Throughput and latency of the native sentence encoder at all-MiniLM-L6-v2's dimensions (6 layers, hidden 384, 12 heads, FFN 1536,
vocab 30522) with recipe weights: 15,000 sentences with fixed-seed lengths in 24..96.

    python tools/bench_text_encode.py [--sentences 15000] [--reps 5] [--out result.json]

Reports sentences/s in both modes (median and min..max over the timed repetitions, the two modes alternating, after a warm-up pass of
each), the share of each kernel family in one corpus run (HIP events around each call of a profiled pass), and the end-to-end latency
of one query (tokenised ids -> embedding on the device, host-synchronised) next to the cosine top-k it feeds."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {"architectures": ["BertModel"], "model_type": "bert", "hidden_size": 384, "num_attention_heads": 12, "intermediate_size": 1536,
       "num_hidden_layers": 6, "max_position_embeddings": 512, "type_vocab_size": 2, "hidden_act": "gelu", "layer_norm_eps": 1e-12,
       "vocab_size": 30522}


def make_model_dir(d, tok_dir):
    import shutil
    from safetensors.numpy import save_file
    from devqa_amd.synth import bert_param_init, bert_param_shapes
    for f in ("tokenizer.json", "tokenizer_config.json", "vocab.txt", "special_tokens_map.json", "modules.json"):
        shutil.copyfile(os.path.join(tok_dir, f), os.path.join(d, f))
    shutil.copytree(os.path.join(tok_dir, "1_Pooling"), os.path.join(d, "1_Pooling"))
    json.dump(CFG, open(os.path.join(d, "config.json"), "w"))
    json.dump({"max_seq_length": 256}, open(os.path.join(d, "sentence_bert_config.json"), "w"))
    save_file({n: bert_param_init(n, s, 5) for n, s in bert_param_shapes(CFG).items()}, os.path.join(d, "model.safetensors"))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def family_times(enc, ids):
    """ms per kernel family over one corpus run: every library call of the pass bracketed by HIP events"""
    from devqa_amd import lib
    fam = {"text_embed_ln": "embed_ln", "gemm": "gemm", "attention": "attention", "layernorm": "layernorm", "seq_pool": "seq_pool"}
    events, saved = [], {}
    for name, f in fam.items():
        orig = saved[name] = getattr(lib, name)

        def wrap(*a, _o=orig, _f=f, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = _o(*a, **k)
            e1.record()
            events.append((_f, e0, e1))
            return r
        setattr(lib, name, wrap)
    try:
        enc.encode_ids(ids)
        torch.cuda.synchronize()
    finally:
        for name, o in saved.items():
            setattr(lib, name, o)
    out = {}
    for f, e0, e1 in events:
        out[f] = out.get(f, 0.0) + e0.elapsed_time(e1)
    return out


def main(argv=None):
    import tempfile
    p = argparse.ArgumentParser()
    p.add_argument("--sentences", type=int, default=15000)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    import devqa_amd  # noqa: F401
    from devqa_amd import lib
    from devqa_amd.text_encoder import SentenceEncoder
    rng = np.random.default_rng(15000)
    lens = rng.integers(24, 97, a.sentences)
    ids = [rng.integers(0, CFG["vocab_size"], int(n)).tolist() for n in lens]
    res = {"sentences": a.sentences, "tokens": int(lens.sum()), "reps": a.reps}
    with tempfile.TemporaryDirectory() as d:
        make_model_dir(d, os.path.join(ROOT, "tests", "golden", "tiny_minilm"))
        encs = {m: SentenceEncoder(d, "cuda:0", m) for m in ("bf16", "fp32")}
    for e in encs.values():                         # warm-up: one whole corpus each
        e.encode_ids(ids)
    times = {m: [] for m in encs}
    for _ in range(a.reps):                         # alternate the variants
        for m, e in encs.items():
            times[m].append(timed(lambda: e.encode_ids(ids)))
    for m, t in times.items():
        t = np.asarray(t)
        res[m] = {"sent_per_s_median": a.sentences / float(np.median(t)), "sent_per_s_min": a.sentences / float(t.max()),
                  "sent_per_s_max": a.sentences / float(t.min()), "seconds": t.tolist(), "family_ms": family_times(encs[m], ids)}
    # Q = 1: one 40-token query, ids -> device embedding, host-synchronised; and the top-k it feeds (15,000 x 384 corpus, k = 32)
    q = [ids[0][:40]]
    corpus = encs["bf16"].encode_ids(ids)
    inv = lib.row_inv_norm(corpus)
    for m, e in encs.items():
        for _ in range(20):
            e.encode_ids(q)
        lat = np.asarray([timed(lambda: e.encode_ids(q)) for _ in range(100)]) * 1e6
        res[m]["q1_latency_us"] = {"median": float(np.median(lat)), "p10": float(np.percentile(lat, 10)), "p90": float(np.percentile(lat, 90))}
    qe = encs["bf16"].encode_ids(q)
    for _ in range(20):
        lib.cosine_topk(corpus, qe, 32, True, True, corpus_inv_norm=inv)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tk = []
    for _ in range(100):
        e0.record()
        lib.cosine_topk(corpus, qe, 32, True, True, corpus_inv_norm=inv)
        e1.record()
        torch.cuda.synchronize()
        tk.append(e0.elapsed_time(e1) * 1e3)
    res["cosine_topk_us_median"] = float(np.median(tk))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
