"""GPU: a plain `bench.py` run (no --full) on a 2-layer model -- the result line carries the headline only, and two runs with the same
arguments write the same --dump-outputs arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_reproducible_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    dumps = []
    for i in range(2):
        d = tmp_path / ("out%d" % i)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                            "--cycles-per-step", "6", "--layers", "2,2,2", "--dump-outputs", str(d)], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert j["steps"] == 2 and j["warmup"] == 1 and j["value"] > 0 and j["ms_per_step"] > 0
        assert j["unit"] == "cycles/s" and j["higher_is_better"] is True and j["dtype"] == "bf16" and j["config"]["cycles_total"] == 12
        assert not {"roofline", "roofline_hbm", "kernels", "strong", "dense_ffn", "configs", "cpu_baseline", "parity"} & set(j)
        dumps.append({f[:-4]: np.load(str(d / f)) for f in sorted(os.listdir(str(d)))})
    a, b = dumps
    assert set(a) == {"accuracy", "ft_steps", "final_loss", "ft_losses", "post_edit_tokens", "pre_edit_tokens"}
    assert a["accuracy"].shape == (6, 12) and a["ft_losses"].shape == (6, 25) and a["post_edit_tokens"].shape[:2] == (6, 12)
    assert all(v.dtype == np.float32 for v in a.values()) and (a["ft_steps"] >= 1).all()
    for name in a:
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
