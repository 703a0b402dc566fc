"""Builds the stored IKE / dataset-builder corpus with the native sentence encoder: training records (JSON) -> build_ike_corpus ->
save_corpus .npz {sentences, images, prompts, embeddings} (R/easyeditor/models/ike/util.py:54-86 does this step with
sentence_transformers and pickles the dict).

    python tools/encode_corpus.py --records train.json --sentence_model_path <all-MiniLM-L6-v2 dir> --out vqa_embeddings.npz

Records are either training records {prompt, target, rephrase_prompt, locality_prompt, locality_ground_truth, image_path,
rephrase_image_path, locality_image_path} or the datasets' raw records {src, alt, rephrase, loc, loc_ans, image, image_rephrase, m_loc}."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RAW_KEYS = {"prompt": "src", "target": "alt", "rephrase_prompt": "rephrase", "locality_prompt": "loc", "locality_ground_truth": "loc_ans",
            "image_path": "image", "rephrase_image_path": "image_rephrase", "locality_image_path": "m_loc"}


def to_training_record(d):
    return d if "prompt" in d else {k: d[v] for k, v in RAW_KEYS.items()}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--records", required=True, help="JSON list of records (or {'raw': [...]})")
    p.add_argument("--sentence_model_path", required=True, help="BERT-family sentence-encoder directory")
    p.add_argument("--out", required=True, help=".npz to write")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("-n", type=int, default=None, help="first n records only")
    a = p.parse_args(argv)
    import devqa_amd  # noqa: F401
    from devqa_amd.dataset.vllm import save_corpus
    from devqa_amd.editor.vllm_editors.ike_vl.ike_vl import build_ike_corpus
    from devqa_amd.text_encoder import SentenceEncoder
    with open(a.records) as f:
        recs = json.load(f)
    if isinstance(recs, dict):
        recs = recs["raw"]
    recs = [to_training_record(d) for d in recs[:a.n]]
    enc = SentenceEncoder(a.sentence_model_path, a.device, a.dtype)
    corpus = build_ike_corpus(recs, enc.encode)
    save_corpus(a.out, corpus)
    print("%d sentences x %d -> %s" % (corpus["embeddings"].shape + (a.out,)))


if __name__ == "__main__":
    main()
