"""GPU: the native sentence encoder (de-vqa_amd/text_encoder.py) against float64.

Bars are the README's: fp32 ("faithful") mode 1e-5, bf16 mode 1e-2, both as max |diff| relative to the reference tensor's max |value|
(text_encoder_ref.rel_err).  The references are the committed float64 transformers.BertModel goldens of the tiny_minilm fixture and,
for the MiniLM-sized layer, the numpy restatement that tests/test_text_encoder_cpu.py pins to those goldens at 1e-10.

What each mode can see (distances of the wrong variants on the golden sentences, tests/test_text_encoder_cpu.py): a tanh GELU lies
1.2e-4 and a LayerNorm eps of 1e-5 lies 6.5e-5 from the right embedding -- both outside the fp32 bar and far inside the bf16 bar, so
only the fp32-mode cases can tell them apart; bf16 mode cannot see those two.  Mean pooling without the specials (0.72), CLS pooling
(0.76) and a missing token-type row (0.88) are outside both bars."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import text_encoder_ref as T

pytestmark = pytest.mark.gpu

BAR = {"fp32": 1e-5, "bf16": 1e-2}


@pytest.fixture(scope="module")
def gold():
    j = json.load(open(os.path.join(T.GOLD, "tiny_text_goldens.json")))
    z = np.load(os.path.join(T.GOLD, "tiny_text_goldens.npz"))
    return j, z


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def enc(request):
    import devqa_amd  # noqa: F401
    from devqa_amd.text_encoder import SentenceEncoder
    return SentenceEncoder(T.TINY, "cuda:0", request.param)


def test_tiny_model_matches_goldens(enc, gold):
    j, z = gold
    bar = BAR[enc.dtype]
    assert enc.dim == 48 and enc.pooling == "mean" and enc.normalize and enc.max_seq_length == 96
    assert enc.tokenize(j["sentences"]) == j["ids"]
    e = enc.encode(j["sentences"])
    assert e.dtype == np.float32 and e.shape == (12, 48)
    err = T.rel_err(e, z["emb_mean_norm"])
    print("tiny %s: embedding rel err %.3g" % (enc.dtype, err))
    assert err < bar
    ed = enc.encode_device(j["sentences"])
    assert ed.is_cuda and ed.dtype == torch.float32 and ed.is_contiguous() and np.array_equal(ed.cpu().numpy(), e)
    # per-layer hidden states of sentence 0 (embedding output, layer 0, layer 1)
    hid = enc.hidden_states(j["sentences"][:1])
    assert len(hid) == 3
    for i, h in enumerate(hid):
        err = T.rel_err(h.cpu().numpy(), z["hidden0_%d" % i])
        print("tiny %s: hidden %d rel err %.3g" % (enc.dtype, i, err))
        assert err < bar, i


def test_long_sentence_is_truncated(enc, gold):
    j, z = gold
    long_s = j["sentences"][-1]
    ids = enc.tokenize([long_s])[0]
    assert len(ids) == 96 == j["max_seq_length"] and ids == j["ids"][-1]
    a, b = enc.encode_device([long_s]), enc.encode_ids([j["ids"][-1]])
    assert torch.equal(a, b)                                    # the over-long sentence IS its truncated form
    assert T.rel_err(a.cpu().numpy(), z["emb_mean_norm"][-1:]) < BAR[enc.dtype]


def test_alone_equals_in_batch(enc, gold):
    j, z = gold
    full = enc.encode(j["sentences"])
    for i in (0, 8, 11):        # 38 tokens, 3 tokens, 96 tokens
        alone = enc.encode(j["sentences"][i:i + 1])
        assert T.rel_err(alone, full[i:i + 1]) < BAR[enc.dtype], i
    # several passes (a pass of at most 128 token rows) give what one pass gives, to the same bar
    old, enc.max_rows = enc.max_rows, 128
    try:
        assert len(enc._passes(j["ids"])) > 3
        assert T.rel_err(enc.encode(j["sentences"]), full) < BAR[enc.dtype]
    finally:
        enc.max_rows = old


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_cls_pooling_variant_and_plain_hf_dir(mode, gold, tmp_path):
    import devqa_amd  # noqa: F401
    from devqa_amd.text_encoder import SentenceEncoder
    j, z = gold
    e = SentenceEncoder(T.cls_variant_dir(tmp_path), "cuda:0", mode)
    assert e.pooling == "cls" and not e.normalize
    assert T.rel_err(e.encode(j["sentences"]), z["emb_cls"]) < BAR[mode]
    # a plain HF directory (`bert.` keys, pooler, no modules.json): mean pooling without Normalize, 128 positions
    p = SentenceEncoder(T.plain_hf_dir(tmp_path), "cuda:0", mode)
    assert p.pooling == "mean" and not p.normalize and p.max_seq_length == 128
    W, cfg = T.load_tiny_weights(), json.load(open(os.path.join(T.TINY, "config.json")))
    ids = j["ids"][:11]
    assert T.rel_err(p.encode_ids(ids).cpu().numpy(), T.encode_ref(W, cfg, ids, "mean", False)) < BAR[mode]


# ---- MiniLM's real layer shape -------------------------------------------------------------------------------------------------
REAL = {"architectures": ["BertModel"], "model_type": "bert", "hidden_size": 384, "num_attention_heads": 12, "intermediate_size": 1536,
        "num_hidden_layers": 1, "max_position_embeddings": 128, "type_vocab_size": 2, "hidden_act": "gelu", "layer_norm_eps": 1e-12,
        "vocab_size": 211}


@pytest.fixture(scope="module")
def real_layer(tmp_path_factory):
    """one all-MiniLM-L6-v2-shaped layer with recipe weights, 64 sentences of 5..120 tokens, and its float64 embeddings / last states"""
    import devqa_amd  # noqa: F401
    from safetensors.numpy import save_file
    from devqa_amd.synth import bert_param_init, bert_param_shapes
    d = str(tmp_path_factory.mktemp("minilm_layer"))
    for f in ("tokenizer.json", "tokenizer_config.json", "vocab.txt", "special_tokens_map.json", "modules.json"):
        shutil.copyfile(os.path.join(T.TINY, f), os.path.join(d, f))
    shutil.copytree(os.path.join(T.TINY, "1_Pooling"), os.path.join(d, "1_Pooling"))
    json.dump(REAL, open(os.path.join(d, "config.json"), "w"))
    W = {n: bert_param_init(n, s, 5) for n, s in bert_param_shapes(REAL).items()}
    save_file(W, os.path.join(d, "model.safetensors"))
    rng = np.random.default_rng(64)
    lens = [5, 120, 64, 65] + rng.integers(5, 121, 60).tolist()
    ids = [rng.integers(0, REAL["vocab_size"], n).tolist() for n in lens]
    ids[0][0], ids[1][0] = 0, REAL["vocab_size"] - 1
    hid = []
    ref = T.encode_ref(W, REAL, ids, "mean", True, hidden=hid)
    return d, ids, ref, np.concatenate([h[-1] for h in hid])


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_minilm_layer_shape(mode, real_layer):
    from devqa_amd.text_encoder import SentenceEncoder
    d, ids, ref, last = real_layer
    e = SentenceEncoder(d, "cuda:0", mode)
    assert (e.D, e.H, e.dh, e.max_seq_length) == (384, 12, 32, 128)
    err = T.rel_err(e.encode_ids(ids).cpu().numpy(), ref)
    hidden = []
    with torch.cuda.device(e.device):
        e._forward(ids, hidden)
    herr = T.rel_err(hidden[-1].cpu().numpy(), last)
    print("MiniLM layer %s: embedding rel err %.3g, last hidden state rel err %.3g" % (mode, err, herr))
    assert err < BAR[mode] and herr < BAR[mode]


# ---- retrieval through IKEvl, wiring of LTEvl --------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["fp32", "bf16"])
def vllm(request, gold_dir):
    import devqa_amd  # noqa: F401
    from devqa_amd.editor.vllms_for_edit.blip2.blip2 import BLIP2OPTForEdit
    return BLIP2OPTForEdit(os.path.join(gold_dir, "tiny_blip2"), "cuda:0", dtype=request.param), request.param


def test_ike_retrieval_from_a_model_directory(vllm, gold, gold_dir):
    """24 corpus sentences (build_ike_corpus over the 8 training records), the 8 IKE queries, k = 3; the encoder is built by IKEvl
    from IKEvlConfig.sentence_model_path alone, in the wrapper's mode.  The golden tool found every float64 gap between rank 3 and
    rank 4 above 1e-4 (the smallest is 1.6e-4), so no query is excluded."""
    from devqa_amd.editor.vllm_editors.ike_vl.ike_vl import IKEvl, IKEvlConfig, build_ike_corpus
    from devqa_amd.text_encoder import SentenceEncoder
    vl, mode = vllm
    j, z = gold
    rec = json.load(open(os.path.join(gold_dir, "evqa8_records.json")))
    builder = SentenceEncoder(T.TINY, "cuda:0", mode)
    corpus = build_ike_corpus(T.train_records(rec["raw"]), builder.encode)
    assert corpus["embeddings"].shape == (24, 48) and T.rel_err(corpus["embeddings"], z["corpus_emb"]) < BAR[mode]
    ed = IKEvl(vl, IKEvlConfig("blip2-opt-2.7b", k=3, sentence_model_path=T.TINY), "cuda:0", corpus)
    assert isinstance(ed.encode, SentenceEncoder) and ed.encode.dtype == mode
    sims = z["emb_mean_norm"][:8] @ z["corpus_emb"].T                     # float64, unit vectors on both sides
    excluded = [q for q in range(8) if j["gap34"][q] <= 1e-4]
    assert len(excluded) <= 1
    for q, r in enumerate(rec["records"]):
        req = r["requests"][0]
        icl = ed.retrieve(req["prompt"], req["target_new"])
        assert len(icl) == 4 and icl[3] == j["sentences"][q]
        got = [corpus["sentences"].index(s) for s in icl[:3]]
        if mode == "fp32":
            if q not in excluded:
                assert got == j["top3"][q], q
        else:   # ids may differ at near-ties; the scores of what was returned are the float64 top-k scores to 2e-2
            assert np.abs(sims[q, got] - z["top3_scores"][q]).max() < 2e-2, q


def test_lte_pool_filled_by_the_native_encoder(vllm, gold_dir, in_gold_dir):
    from devqa_amd.editor.vllm_editors.lte_vl.lte_vl import LTEvl, LTEvlConfig
    from devqa_amd.text_encoder import SentenceEncoder
    vl, mode = vllm
    cfg = LTEvlConfig("blip2-opt-2.7b", LTEvlConfig.TrainConfig(5e-6, 1.0, 1.0, 1.0), "language_model", T.TINY, 48, 0.6)
    ed = LTEvl(vl, cfg, "cuda:0")
    try:
        assert isinstance(ed.encode, SentenceEncoder) and ed.encode.dtype == mode
        req = json.load(open(os.path.join(gold_dir, "evqa8_records.json")))["records"][0]["requests"][0]
        ed.edit_one_piece(req)
        want = ed.encode.encode_device([req["prompt"] + " " + req["target_new"]])
        assert ed.text_retr_pool.shape == (1, 48) and ed.text_retr_pool.is_cuda and torch.equal(ed.text_retr_pool, want)
        hit, _, val = ed.retrieval([req["prompt"]])                    # float64 cosine of the two sentences: 0.996
        assert hit[0] is req and float(val[0, 0]) > 0.6
        cfg.retrieval_embed_dim = 32
        with pytest.raises(RuntimeError, match="expected \\[n, 32\\]"):
            ed._embed(["x"])
    finally:
        ed.restore_to_original_model()
        vl.get_llm_outpt = ed.original_get_llm_outpt
