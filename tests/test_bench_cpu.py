"""bench.py host logic without a GPU: the option defaults, the --dump-outputs file set, and the input preparation (pixels computed on a
thread pool) against the one-image-at-a-time form."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_plain_run_is_the_default():
    a = bench.parse_args([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def _result(i):
    from devqa_amd.batched import LOC_ORDER

    def probe(acc, ids, pre=None):
        p = {"acc": acc, "predict_after_edit": " ".join(str(t) for t in ids)}
        if pre is not None:
            p["predict_before_edit"] = " ".join(str(t) for t in pre)
        return p
    return {"reliability": [dict(probe(1.0, [5, 6 + i]), edit_time=0.01 * (i + 1))],
            "generality": {"text_rephrase": [probe(0.5, [7])], "image_rephrase": [probe(0.0, [8, 9, 10])]},
            "locality": {n: [probe(1.0, [11 + j], [11 + j, 3])] for j, n in enumerate(LOC_ORDER)}}


def test_dump_outputs_files(tmp_path):
    import devqa_amd  # noqa: F401
    outs = [_result(i) for i in range(3)]
    metas = [(25, 0.5), (3, 0.25), (25, 0.125)]
    losses = np.arange(75, dtype=np.float32).reshape(3, 25)
    bench.dump_outputs(str(tmp_path / "o"), outs, metas, np.array([25, 3, 25], np.int32), losses)
    got = {f[:-4]: np.load(str(tmp_path / "o" / f)) for f in os.listdir(str(tmp_path / "o"))}
    assert set(got) == {"accuracy", "ft_steps", "final_loss", "ft_losses", "post_edit_tokens", "pre_edit_tokens"}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["accuracy"].shape == (3, 12) and list(got["accuracy"][0, :3]) == [1.0, 0.5, 0.0]
    assert list(got["ft_steps"]) == [25, 3, 25] and list(got["final_loss"]) == [0.5, 0.25, 0.125]
    np.testing.assert_array_equal(got["ft_losses"], losses)
    assert got["post_edit_tokens"].shape == (3, 12, 3) and list(got["post_edit_tokens"][1, 0]) == [5, 7, -1]
    assert got["pre_edit_tokens"].shape == (3, 9, 2) and list(got["pre_edit_tokens"][0, 8]) == [19, 3]


def _fake_leg(scaling, world, rank, monkeypatch):
    """A Leg with its input side only (host tensors): make_batches without a model or a GPU."""
    from devqa_amd import blip2_spec
    from devqa_amd.batched import copy_sample, shard_range
    from devqa_amd.editor.vllms_for_edit.blip2.blip2 import Blip2ImagePreprocessor
    from devqa_amd.synth import evqa_cycles, synth_image_u8
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    leg = bench.Leg.__new__(bench.Leg)
    leg.args = bench.parse_args(["--cycles-per-step", "5", "--scaling", scaling, "--strong-cycles", "23"])
    leg.rank, leg.world, leg.dev = rank, world, "cpu"
    leg.vllm = types.SimpleNamespace(image_processor=Blip2ImagePreprocessor(224))
    leg.cfg = blip2_spec.BLIP2_OPT_2_7B
    leg.copy_sample, leg.shard_range, leg._evqa_cycles, leg._synth_image_u8, leg._img_cache = (copy_sample, shard_range, evqa_cycles,
                                                                                               synth_image_u8, {})
    return leg


def test_prefetched_pixels_equal_the_serial_form(monkeypatch):
    """Every image of the warm-up and timed batches is the preprocessor's output for its (seed, sample, tag), bit for bit -- for both
    scaling modes and a rank other than 0 (the sample offsets differ)."""
    import devqa_amd  # noqa: F401
    from devqa_amd.synth import synth_image_u8
    for scaling, world, rank in (("weak", 2, 1), ("strong", 3, 2)):
        leg = _fake_leg(scaling, world, rank, monkeypatch)
        warm, timed, _, _ = leg.make_batches(3, 2, scaling)
        lo, hi = leg.shard_range(15, rank, world)
        assert len(warm) == 2 and sum(len(b[1]) for b in timed) == (15 if scaling == "weak" else hi - lo)
        proc = leg.vllm.image_processor
        by_id = {id(v): k for k, v in leg._img_cache.items()}
        n = 0
        for _, eds in warm + timed:
            for c in eds:
                for it in [c["requests"][0]] + [v[0] for sec in ("generality", "locality") for v in c[sec].values()]:
                    if it["image"] is None:
                        continue
                    s, tag = by_id[id(it["image"])]
                    assert torch.equal(it["image"], torch.from_numpy(proc(synth_image_u8(s, tag, 224, leg.args.seed))))
                    n += 1
        assert n == 9 * (len(warm[0][1]) * len(warm) + sum(len(b[1]) for b in timed))
