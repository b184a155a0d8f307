"""CPU: the parts of bench.py that do not need a GPU -- the HBM-traffic record is only reported for the kernel source,
shape and launch geometry it was measured for, and the committed record matches the committed kernel sources."""
import importlib.util
import json
import os

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _records():
    recs = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    return [recs] if isinstance(recs, dict) else recs


def test_committed_traffic_record_belongs_to_the_committed_kernel_sources():
    bench = _bench()
    recs = _records()
    assert recs[0]["rows"] == 1000000 and recs[0]["K"] == 128          # the headline shape comes first
    for rec in recs:
        assert rec["source_sha256"] == bench.kernel_source_digest(rec["kernel"]), \
            "the kernel's source file / fsnap_device_common.h changed after the PMC passes: re-run scripts/pmc_record_all.sh"
        info = {"workgroups": rec["workgroups"], "threads": rec["threads"], "chunks_per_wave": rec["chunks_per_wave"]}
        traffic, source = bench.recorded_traffic(rec["rows"], rec["K"], info, rec["kernel"])
        assert traffic == rec["hbm_bytes_per_launch"] and "FETCH_SIZE" in source
    # headline kernel: 1.02 x the algorithmic bytes, the rows are read once
    rec = recs[0]
    assert 1.0 <= rec["hbm_bytes_per_launch"] / rec["algorithmic_bytes_per_launch"] < 1.05


def test_traffic_is_null_for_any_other_shape_geometry_or_kernel():
    bench = _bench()
    rec = _records()[0]
    info = {"workgroups": rec["workgroups"], "threads": rec["threads"], "chunks_per_wave": rec["chunks_per_wave"]}
    for change in ({"rows": rec["rows"] + 1}, {"K": 96}, {"kernel": "fsnap_syrk_tiled"}):
        args = {"rows": rec["rows"], "K": rec["K"], "kernel": rec["kernel"], **change}
        traffic, why = bench.recorded_traffic(args["rows"], args["K"], info, args["kernel"])
        assert traffic is None and "recorded for" in why
    other = dict(info, chunks_per_wave=info["chunks_per_wave"] + 1)
    assert bench.recorded_traffic(rec["rows"], rec["K"], other, rec["kernel"])[0] is None


def test_dump_outputs_writes_float64_files_within_the_size_limit(tmp_path):
    import numpy as np

    bench = _bench()
    beta = np.arange(5.0)
    paths = bench.dump_outputs(str(tmp_path / "small"), {"beta": beta, "rank": [5]})
    assert paths == ["beta", "rank"]
    got = np.load(tmp_path / "small" / "beta.npy")
    assert got.dtype == np.float64 and np.array_equal(got, beta)
    # a set above the limit: the largest array becomes a fixed sample (the same positions on every run) plus its positions
    G = np.random.default_rng(3).standard_normal((3000, 3000))
    bench.DUMP_MAX_BYTES = 1_000_000
    names = bench.dump_outputs(str(tmp_path / "big"), {"G": G, "c": beta})
    assert names == ["G_sample", "G_sample_index", "c"]
    total = sum(os.path.getsize(tmp_path / "big" / (n + ".npy")) for n in names)
    assert total <= 1_000_000 + 3 * 128                               # (npy headers)
    idx = np.load(tmp_path / "big" / "G_sample_index.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "big" / "G_sample.npy"), G.ravel()[idx])
    bench.dump_outputs(str(tmp_path / "again"), {"G": G, "c": beta})
    assert np.array_equal(np.load(tmp_path / "again" / "G_sample_index.npy"), idx)


def test_steps_must_be_positive():
    import pytest

    bench = _bench()
    assert bench.parse(["--steps", "7", "--warmup", "2"]).steps == 7
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])
