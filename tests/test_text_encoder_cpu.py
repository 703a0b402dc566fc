"""CPU: the sentence encoder's fixture, loader, C-ABI surface and wiring (no GPU: nothing here launches a kernel).

The goldens (tests/golden/tiny_text_goldens.*, tools/make_goldens_text_encoder.py) are float64 transformers.BertModel outputs on the
tiny_minilm fixture; tests/text_encoder_ref.py restates the arithmetic in numpy so the GPU tests need no HF model run.  Both must
reproduce the committed numbers to 1e-10.

How far the wrong variants of the restatement lie from the right one on the 12 golden sentences (max-abs, relative to the embedding's
max-abs; printed by the golden tool) -- what a comparison at the fp32 bar (1e-5) can and a comparison at the bf16 bar (1e-2) cannot see:
    tanh GELU                     1.2e-4
    LayerNorm eps 1e-5            6.5e-5
    mean without [CLS] / [SEP]    7.2e-1
    CLS pooling instead of mean   7.6e-1
    no token-type row             8.8e-1"""
import ctypes
import json
import os
import re
import shutil
from types import SimpleNamespace

import numpy as np
import pytest

import text_encoder_ref as T

ROOT = T.ROOT


@pytest.fixture(scope="module")
def gold():
    j = json.load(open(os.path.join(T.GOLD, "tiny_text_goldens.json")))
    z = np.load(os.path.join(T.GOLD, "tiny_text_goldens.npz"))
    cfg = json.load(open(os.path.join(T.TINY, "config.json")))
    return j, z, cfg, T.load_tiny_weights()


def test_restatement_reproduces_goldens(gold):
    j, z, cfg, W = gold
    hid = []
    e = T.encode_ref(W, cfg, j["ids"], "mean", True, hidden=hid)
    assert np.abs(e - z["emb_mean_norm"]).max() < 1e-10
    assert np.abs(T.encode_ref(W, cfg, j["ids"], "cls", False) - z["emb_cls"]).max() < 1e-10
    for i, h in enumerate(hid[0]):
        assert np.abs(h - z["hidden0_%d" % i]).max() < 1e-10
    assert np.abs(np.linalg.norm(e, axis=1) - 1).max() < 1e-12
    # the wrong variants are where the docstring says: each beyond the fp32 bar, the first two inside the bf16 bar
    d = {w: T.rel_err(T.encode_ref(W, cfg, j["ids"], "mean", True, wrong=(w,)), e) for w in ("tanh_gelu", "eps1e-5", "no_specials", "cls", "no_type")}
    assert 5e-5 < d["tanh_gelu"] < 1e-2 and 2e-5 < d["eps1e-5"] < 1e-2 and min(d["no_specials"], d["cls"], d["no_type"]) > 0.1, d


def test_transformers_bert_reproduces_goldens(gold):
    import torch
    from transformers import BertConfig, BertModel
    j, z, cfg, W = gold
    model = BertModel(BertConfig(**cfg), add_pooling_layer=False).double().eval()
    model.load_state_dict({k: torch.from_numpy(v).double() for k, v in W.items()}, strict=False)
    for s, want_mean, want_cls in zip(j["ids"], z["emb_mean_norm"], z["emb_cls"]):
        with torch.no_grad():
            h = model(input_ids=torch.tensor([s])).last_hidden_state[0].numpy()
        e = h.sum(0) / len(s)
        assert np.abs(e / np.linalg.norm(e) - want_mean).max() < 1e-10 and np.abs(h[0] - want_cls).max() < 1e-10


def test_fixture_tokenizer_and_recipe(gold):
    from transformers import AutoTokenizer
    import devqa_amd  # noqa: F401
    from devqa_amd.synth import bert_param_init, bert_param_shapes
    j, _, cfg, W = gold
    tok = AutoTokenizer.from_pretrained(T.TINY)
    ids = tok(j["sentences"], add_special_tokens=True, truncation=True, max_length=j["max_seq_length"], padding=False)["input_ids"]
    assert ids == j["ids"]
    cls, sep = tok.cls_token_id, tok.sep_token_id
    assert all(s[0] == cls and s[-1] == sep for s in ids)
    assert [len(s) for s in ids[8:11]] == [3, 4, 8] and len(ids[11]) == j["max_seq_length"] < j["long_untruncated_tokens"]
    assert tok.unk_token_id not in sum(ids, [])
    shapes = bert_param_shapes(cfg)
    assert set(shapes) == set(W)
    for n in ("embeddings.LayerNorm.weight", "encoder.layer.1.output.dense.weight"):
        assert np.array_equal(W[n], bert_param_init(n, shapes[n], j["seed"]))


def test_layout_parsing(tmp_path):
    import devqa_amd  # noqa: F401
    from devqa_amd.text_encoder import is_bert_dir, load_bert_state, read_model_layout
    cfg, msl, pooling, norm = read_model_layout(T.TINY)
    assert (msl, pooling, norm) == (96, "mean", True) and cfg["hidden_size"] == 48
    assert read_model_layout(T.cls_variant_dir(tmp_path))[1:] == (96, "cls", False)
    plain = T.plain_hf_dir(tmp_path)
    assert read_model_layout(plain)[1:] == (128, "mean", False)            # max_position_embeddings, mean, no Normalize
    assert is_bert_dir(T.TINY) and is_bert_dir(plain) and not is_bert_dir(None) and not is_bert_dir(str(tmp_path / "nowhere"))
    assert not is_bert_dir("sentence-transformers/multi-qa-mpnet-base-dot-v1")
    # `bert.` prefix stripped, pooler and position_ids ignored: the same tensors as the sentence-transformers directory
    a, b = load_bert_state(T.TINY), load_bert_state(plain)
    assert set(a) == set(b) == set(T.load_tiny_weights()) and all(np.array_equal(a[k].numpy(), b[k].numpy()) for k in a)
    # max pooling, and a pooling the kernels do not have
    d = T.cls_variant_dir(tmp_path / "m")
    pc = os.path.join(d, "1_Pooling_cls", "config.json")
    p = json.load(open(pc))
    json.dump(dict(p, pooling_mode_cls_token=False, pooling_mode_max_tokens=True), open(pc, "w"))
    assert read_model_layout(d)[2] == "max"
    json.dump(dict(p, pooling_mode_cls_token=False, pooling_mode_mean_sqrt_len_tokens=True), open(pc, "w"))
    with pytest.raises(NotImplementedError, match="pooling"):
        read_model_layout(d)


def _copy_with_config(tmp_path, name, **changes):
    dst = os.path.join(str(tmp_path), name)
    shutil.copytree(T.TINY, dst)
    cfg = json.load(open(os.path.join(dst, "config.json")))
    cfg.update(changes)
    json.dump(cfg, open(os.path.join(dst, "config.json"), "w"))
    return dst


def test_loader_errors(tmp_path):
    import devqa_amd  # noqa: F401
    from devqa_amd.text_encoder import SentenceEncoder
    with pytest.raises(NotImplementedError, match="mpnet"):
        SentenceEncoder(_copy_with_config(tmp_path, "mpnet", model_type="mpnet"), "cpu")
    with pytest.raises(NotImplementedError, match="relative_key"):
        SentenceEncoder(_copy_with_config(tmp_path, "rel", position_embedding_type="relative_key"), "cpu")
    with pytest.raises(NotImplementedError, match="gelu_new"):
        SentenceEncoder(_copy_with_config(tmp_path, "act", hidden_act="gelu_new"), "cpu")
    d = _copy_with_config(tmp_path, "noweights")
    os.remove(os.path.join(d, "model.safetensors"))
    with pytest.raises(FileNotFoundError, match="model.safetensors"):
        SentenceEncoder(d, "cpu")
    # host checks before any launch (the tables live on the CPU here: nothing is launched): an id beyond the word table, too many tokens
    enc = SentenceEncoder(T.TINY, "cpu", "fp32")
    assert enc.dim == 48 and enc.max_seq_length == 96 and enc.pooling == "mean" and enc.normalize
    with pytest.raises(ValueError, match="outside the word table"):
        enc.encode_ids([[2, enc.V, 3]])
    with pytest.raises(ValueError, match="outside the word table"):
        enc.encode_ids([[2, -1, 3]])
    with pytest.raises(ValueError, match="max_seq_length"):
        enc.encode_ids([[2] + [10] * 96 + [3]])
    long_ids = enc.tokenize(["pans " * 300])[0]
    assert len(long_ids) == 96 and long_ids[0] == enc.tokenizer.cls_token_id and long_ids[-1] == enc.tokenizer.sep_token_id
    assert enc._passes([[1] * 60] * 5) == [(0, 5)]
    enc.max_rows = 128
    assert enc._passes([[1] * 60] * 5) == [(0, 2), (2, 4), (4, 5)]


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
_OPS = "tests/test_text_ops_gpu.py::"
COVERED_BY = {
    "devqa_text_embed_ln": _OPS + "test_embed_ln",
    "devqa_text_embed_ln_f32": _OPS + "test_embed_ln",
    "devqa_seq_pool": _OPS + "test_seq_pool",
}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    so = os.path.join(ROOT, "de-vqa_amd", "csrc", "libdevqa_hip.so")
    if not os.path.exists(so):
        g.build()
    return so


def test_text_exports_header_binding_and_tests(built):
    import ast
    import devqa_amd  # noqa: F401
    from devqa_amd import lib
    hdr = open(os.path.join(ROOT, "include", "devqa_text.h")).read()
    names = set(re.findall(r"\b(devqa_[a-z0-9_]+)\s*\(", hdr))
    assert names == set(lib.EXPORTS_TEXT) == set(COVERED_BY) and len(lib.EXPORTS_TEXT) == len(names)
    L = lib.load()
    so = ctypes.CDLL(built)
    for n in names:
        assert hasattr(so, n) and getattr(L, n).argtypes is not None, n
    # the existing lists are untouched by the new names, and the ABI version did not move
    main_hdr = open(os.path.join(ROOT, "include", "devqa.h")).read()
    for n in names:
        assert n not in lib.EXPORTS and n not in main_hdr
    assert "devqa_text" not in main_hdr and "devqa_seq_pool" not in main_hdr
    assert L.devqa_abi_version() == 1
    for sym, where in COVERED_BY.items():
        path, _, func = where.partition("::")
        tree = ast.parse(open(os.path.join(ROOT, *path.split("/"))).read())
        assert func in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}, (sym, where)


def test_text_argument_validation_without_gpu(built):
    so = ctypes.CDLL(built)
    so.devqa_last_error.restype = ctypes.c_char_p
    F, one = ctypes.c_float(1e-12), ctypes.c_void_p(64)       # a non-null pointer that a rejected call never follows
    assert so.devqa_text_embed_ln(None, None, None, None, None, None, None, 1, 48, 10, 10, F, None, None, None) == -1
    assert b"null" in so.devqa_last_error()
    assert so.devqa_text_embed_ln_f32(one, one, one, one, one, one, one, 1, 48, 10, 10, F, None, None, None) == -1   # no output
    for bad_d in (46, 0, 4100):
        assert so.devqa_text_embed_ln(one, one, one, one, one, one, one, 1, bad_d, 10, 10, F, one, one, None) == -2
        assert b"D=%d" % bad_d in so.devqa_last_error()
    assert so.devqa_text_embed_ln_f32(one, one, one, one, one, one, one, 1, 48, 0, 10, F, one, one, None) == -2
    assert so.devqa_seq_pool(None, one, one, 1, 1, 48, 0, 0, one, None) == -1
    assert so.devqa_seq_pool(one, one, one, 1, 1, 48, 3, 0, one, None) == -1 and b"mode" in so.devqa_last_error()
    assert so.devqa_seq_pool(one, one, one, 1, 1, 50, 0, 0, one, None) == -2
    assert so.devqa_seq_pool(one, one, one, 4, 0, 48, 0, 1, one, None) == 0          # nothing to do: no launch


# ---- wiring: without an encoder and without a model directory the constructors raise what they raised before -----------------------
def _stub_vllm():
    import devqa_amd  # noqa: F401
    from devqa_amd.editor.vllms_for_edit.base import BaseVLLMForEdit

    class Stub(BaseVLLMForEdit):
        def __init__(self):
            self.model = SimpleNamespace(config=SimpleNamespace(is_encoder_decoder=False))

        def set_device(self, device):
            self.device = device

        def get_llm_tokenizer(self): return None
        def get_llm_input_embeds(self, texts, imgs=None): return None
        def get_llm_outpt(self, input_embeds, vt_range=None): return None
        def get_img_special_token_str(self): return ""
        def get_img_special_token_id(self): return 0
        def get_img_token_n(self): return 0
        def is_q_former_based(self): return False
    return Stub()


def test_editors_without_encoder_raise_as_before(tmp_path):
    import devqa_amd  # noqa: F401
    from devqa_amd.dataset.vllm import EVQA
    from devqa_amd.editor.vllm_editors.ike_vl.ike_vl import IKEvl, IKEvlConfig
    from devqa_amd.editor.vllm_editors.lte_vl.lte_vl import LTEvl, LTEvlConfig
    corpus = {"sentences": ["a"], "embeddings": np.zeros((1, 4), np.float32)}
    assert IKEvlConfig("blip2-opt-2.7b").sentence_model_path is None
    msg = "IKEvl needs the stored corpus {sentences, embeddings} and a sentence encoder"
    for cfg, c in ((IKEvlConfig("blip2-opt-2.7b"), corpus), (IKEvlConfig("blip2-opt-2.7b", sentence_model_path=str(tmp_path / "nowhere")), corpus),
                   (IKEvlConfig("blip2-opt-2.7b", sentence_model_path=T.TINY), None)):
        with pytest.raises(RuntimeError) as e:
            IKEvl(_stub_vllm(), cfg, "cpu", c, None)
        assert str(e.value) == msg
    lcfg = LTEvlConfig("blip2-opt-2.7b", LTEvlConfig.TrainConfig(5e-6, 1.0, 1.0, 1.0), "language_model",
                       "sentence-transformers/multi-qa-mpnet-base-dot-v1", 768, 0.6)
    with pytest.raises(RuntimeError) as e:
        LTEvl(_stub_vllm(), lcfg, "cpu")
    assert str(e.value) == ("LTEvl needs `encode`: list[str] -> [n, 768] sentence embeddings (the reference uses "
                            "SentenceTransformer('sentence-transformers/multi-qa-mpnet-base-dot-v1'))")
    vqa = tmp_path / "vqa_eval.json"
    vqa.write_text("[]")
    with pytest.raises(RuntimeError) as e:
        EVQA(str(vqa), str(tmp_path))
    assert str(e.value) == "EVQA needs a retriever (the reference's hard-coded SentenceTransformer path does not exist here)"
    with pytest.raises(RuntimeError, match="also needs corpus="):      # a model directory alone: say what is missing
        EVQA(str(vqa), str(tmp_path), sentence_model_path=T.TINY)
    # an encoder of another width than retrieval_embed_dim is refused at construction, not at the first edit
    class Enc48:
        dim = 48

        def __call__(self, s):
            return np.zeros((len(s), 48), np.float32)
    with pytest.raises(RuntimeError, match="48-d embeddings, retrieval_embed_dim is 768"):
        LTEvl(_stub_vllm(), lcfg, "cpu", encode=Enc48())


def test_cli_flag_and_corpus_tool_parse():
    import argparse
    import devqa_amd  # noqa: F401
    from devqa_amd import cli
    a = cli.add_data_args(argparse.ArgumentParser()).parse_args([])
    assert a.sentence_model_path is None and cli.load_encoder(a) is None
    a = cli.add_data_args(argparse.ArgumentParser()).parse_args(["--sentence_model_path", "x"])
    assert a.sentence_model_path == "x"
