"""Host-side pieces of bench.py that need no GPU: the core / thread accounting of the CPU-baseline legs, and the lookup of
the committed PMC passes that `roofline.traffic` / `roofline_hbm.traffic` quote (only for the very workload they were
collected on), and the writer of --dump-outputs."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_env_defaults_are_set_before_torch_is_imported():
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert src.index('os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")') < src.index("import torch")
    main = src[src.index("def main():"):]
    assert "HSA_ENABLE_IPC_MODE_LEGACY" not in main          # (not set late, after the runtime is up)


def test_cpu_accounting_reports_physical_cores_and_threads_separately():
    b = _bench()
    model, physical, logical = b.host_cpu()
    assert 1 <= physical <= logical == (os.cpu_count() or logical)
    quota = b.cpu_quota()
    assert quota is None or quota > 0
    allowed = len(os.sched_getaffinity(0)) if quota is None else min(len(os.sched_getaffinity(0)), max(1, int(quota)))
    assert b.cpu_threads(0) == min(physical, allowed)      # default: one per physical core the process may actually use
    assert b.cpu_threads(3) == min(3, allowed)
    assert b.cpu_threads(10 ** 6) == allowed               # never more than this process may run on at once


def test_pmc_lookup_matches_the_workload_key_only():
    b = _bench()
    key = "cfg1_chair_6m:N=6000000:K=8:SR=80:fp32:jitter=0.3:world=1"
    hit = b.pmc_traffic("k_shade_pairs", key)
    assert hit is not None and 3e9 < hit[0] < 7e9 and hit[1].startswith("profiles/")
    newest = sorted(d for d in os.listdir(os.path.join(ROOT, "profiles")) if d.startswith("r"))[-1]
    assert hit[1].startswith(f"profiles/{newest}/"), hit[1]                        # the newest round's pass wins
    assert b.pmc_traffic("k_shade_pairs", key.replace("world=1", "world=8")) is None
    assert b.pmc_traffic("k_shade_pairs", key.replace("K=8", "K=12")) is None
    q = b.pmc_traffic_sum(b.QUERY_STAGE_KERNELS, key)
    assert q is not None and 5e8 < q[0] < 3e9
    names = {n.split("<")[0].split("::")[-1] for n in q[1]}
    assert {"k_select", "k_expand", "k_knn3"} <= names and "k_shade_pairs" not in names
    assert abs(sum(q[1].values()) - q[0]) < 1.0
    with open(os.path.join(ROOT, q[2])) as f:
        assert json.load(f)["workload_key"] == key


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample_under_the_budget(tmp_path):
    """--dump-outputs: float32 / float64 .npy files; over the budget every large array is cut to the same seeded rows
    on every run (their numbers beside it), small ones stay whole, and the files stay under the budget."""
    import numpy as np
    import torch
    b = _bench()
    g = torch.Generator().manual_seed(1)
    arrays = {"image_rgb": torch.rand(2, 200, 200, 4, generator=g)[..., :3],
              "image_depth": torch.rand(2, 200, 200, generator=g),
              "rays_mask": torch.randint(0, 2, (80000,), generator=g).to(torch.int8),
              "counters": torch.arange(10, dtype=torch.int64)}
    whole = b.dump_outputs(str(tmp_path / "whole"), arrays)
    assert not whole["sampled"]
    assert np.array_equal(np.load(tmp_path / "whole" / "image_rgb.npy"), arrays["image_rgb"].numpy())
    assert np.load(tmp_path / "whole" / "rays_mask.npy").dtype == np.float32
    assert np.load(tmp_path / "whole" / "counters.npy").dtype == np.float64
    budget = 600_000
    for d in ("a", "b"):
        assert b.dump_outputs(str(tmp_path / d), arrays, budget=budget)["sampled"]
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= budget
    for f in files:
        x = np.load(tmp_path / "a" / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, np.load(tmp_path / "b" / f)), f
    rows = np.load(tmp_path / "a" / "image_rgb_rows.npy").astype(np.int64)
    assert 0 < len(rows) < 80000 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "image_rgb.npy"), arrays["image_rgb"].reshape(-1, 3).numpy()[rows])
    assert np.array_equal(np.load(tmp_path / "a" / "counters.npy"), np.arange(10.0))
