"""bench.py on the device, small: the plain line, --dump-outputs, --full — needs an MI355X.

The bench runs in this process (bench.main(argv)) on 96 C2-shaped queries: one plain run
with --dump-outputs shared by the tests, a second one for the run-to-run comparison,
one --full run with the CPU baselines off (they start processes of their own)."""
import json

import numpy as np
import pytest

from oracle import _loader as coracle

pytestmark = pytest.mark.gpu

Q, R, K = 96, 5, 1000
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--queries", str(Q)]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "cpu_baseline", "parity_vs_oracle", "ndcg10", "ndcg10_delta_vs_ref")


def _bench():
    import bench
    return bench


def _load(d):
    return {f.stem: np.load(f) for f in sorted(d.glob("*.npy"))}


@pytest.fixture(scope="module")
def plain(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    res = _bench().main(ARGS + ["--dump-outputs", str(d)])
    return res, d, _load(d)


def test_plain_line(gpu, plain, capfd, monkeypatch):
    """One JSON line on stdout with the headline fields; nothing of --full in it; the
    step runs --warmup times untimed, then --steps times inside the timed loop."""
    bench = _bench()
    calls = []
    step, loop = bench.Pipeline.step, bench.timed_loop
    monkeypatch.setattr(bench.Pipeline, "step",
                        lambda self, timed=False: (calls.append(timed), step(self, timed))[1])
    monkeypatch.setattr(bench, "timed_loop",
                        lambda *a: (calls.append("loop"), loop(*a), calls.append("end"))[1])
    res = bench.main(ARGS)
    assert calls == [False] + ["loop"] + [True] * 3 + ["end"]
    lines = [l for l in capfd.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1 and json.loads(lines[0]) == json.loads(json.dumps(res))
    assert all(k in res for k in HEADLINE)
    assert res["steps"] == 3 and res["warmup"] == 1 and res["full"] is False
    assert res["ms_per_step"] > 0
    # value is the batch over the step time, from the same clock
    assert res["value"] == pytest.approx(Q / (res["ms_per_step"] * 1e-3), rel=1e-3)
    assert not any(k in res for k in FULL_ONLY)
    assert "dumped_outputs" not in res
    assert set(plain[0]["dumped_outputs"]["arrays"]) == set(plain[2])


def test_dump_format_and_size(plain):
    _, d, a = plain
    assert set(a) == {"union_count", "qpp_raw", "qpp_colminmax", "qpp_micro", "sample_queries",
                      "sample_norm_micro", "sample_union_docid", "sample_fused", "sample_perm"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(f.stat().st_size for f in d.iterdir()) <= 64 << 20
    S = 64
    assert a["union_count"].shape == (Q,) and a["qpp_raw"].shape == (Q * R, 13)
    assert a["qpp_micro"].shape == (Q * R, 13) and a["qpp_colminmax"].shape == (2 * R * 13,)
    assert a["sample_fused"].shape == (S, 6, R * K) and a["sample_perm"].shape == (S, 6, R * K)
    assert a["sample_union_docid"].shape == (S, R * K)
    assert a["sample_norm_micro"].shape == (S, R * K)
    q = a["sample_queries"].astype(np.int64)
    assert np.all(np.diff(q) > 0) and q.min() >= 0 and q.max() < Q


def test_dump_identical_run_to_run(gpu, plain, tmp_path):
    """Same arguments, same inputs, same outputs: file for file, byte for byte — whatever
    the number of steps."""
    _bench().main(ARGS[:3] + ["2"] + ARGS[4:] + ["--dump-outputs", str(tmp_path)])
    b = _load(tmp_path)
    assert set(b) == set(plain[2])
    for name, v in plain[2].items():
        assert v.tobytes() == b[name].tobytes(), name


def test_dump_is_the_steps_output(plain):
    """The dumped arrays against the CPU oracle on the regenerated inputs: the .norm.res
    micro-units, the raw QPP predictors, and the ranked lists of the unweighted fusions
    rebuilt from union_docid / fused / perm."""
    bench = _bench()
    a = plain[2]
    qo, qd = bench.nq_qrels()
    off, doc, raw = coracle.synth_runs_nq(0, Q, R, K, bench.SEED, qo, qd)
    norm = coracle.minmax_per_query(raw, off)
    micro = np.array([int(f"{v:.6f}".replace(".", "")) for v in norm], np.int64).reshape(Q, R * K)
    sample = a["sample_queries"].astype(np.int64)
    assert np.array_equal(a["sample_norm_micro"].astype(np.int64), micro[sample])
    nt, tf = bench.text_inputs(0, Q)
    cut = np.arange(Q * R + 1, dtype=np.int64) * 100
    want = coracle.qpp_raw(raw.reshape(Q * R, K)[:, :100].ravel(), cut, np.repeat(nt, R),
                           np.repeat(tf[:, 0], R), np.repeat(tf[:, 1], R))
    np.testing.assert_allclose(a["qpp_raw"], want, rtol=1e-12, atol=1e-15)
    # the column extremes ([min | -max], retriever-major) and the .qpp table of the dumped
    # predictors: the reference's per-file min-max (oracle/ref_port.py) and its "%.6f"
    from oracle import ref_port
    got = a["qpp_raw"]
    for r in range(R):
        col = got[r::R]
        assert np.array_equal(a["qpp_colminmax"][r * 13:(r + 1) * 13], col.min(axis=0))
        assert np.array_equal(a["qpp_colminmax"][(R + r) * 13:(R + r + 1) * 13], -col.max(axis=0))
        norm = ref_port.normalize_qpp({str(q): col[q].tolist() for q in range(Q)}, "minmax")
        table = np.array([[int(f"{v:.6f}".replace(".", "")) for v in norm[str(q)]]
                          for q in range(Q)], np.float64)
        assert np.array_equal(a["qpp_micro"][r::R], table), r
    sc = micro.ravel().astype(np.float64) / 1e6
    for m, name in enumerate(bench.METHODS[:3]):
        ud, uc, perm, fused = coracle.fuse(off, doc, sc, R, name, 60)
        assert np.array_equal(a["union_count"], uc)
        for i, q in enumerate(sample):
            b, n = off[q * R], uc[q]
            pm = a["sample_perm"][i, m, :n].astype(np.int64)
            assert np.array_equal(pm, perm[b:b + n]), (name, q)
            assert a["sample_fused"][i, m, pm].tobytes() == fused[b:b + n].tobytes(), (name, q)
            assert np.array_equal(a["sample_union_docid"][i, :n], ud[b:b + n]), (name, q)
            assert np.all(a["sample_perm"][i, m, n:] == -1)
            assert np.all(a["sample_fused"][i, m, n:] == 0)


def test_full_line(gpu):
    """--full: the same headline fields plus the roofline object and the checks."""
    res = _bench().main(ARGS + ["--full", "--cpu-sample", "0", "--check", "4",
                               "--ndcg-sample", "16"])
    assert all(k in res for k in HEADLINE) and res["full"] is True and res["steps"] == 3
    assert res["parity_vs_oracle"] == {"queries": 4, "bit_exact": True}
    assert res["roofline"]["kernel_ms"] > 0 and res["roofline"]["copy_ceiling_gbs"] > 0
    assert set(res["ndcg10"]) == set(_bench().METHODS)
    assert res["ndcg10_delta_vs_ref"]["queries"] == 16
    assert res["cpu_baseline"] is None
