"""bench.py's options and --dump-outputs writer on the host (CPU): dump_outputs reads the
step's buffers only through .cpu(), so a stand-in pipeline of host tensors exercises
the sample, the padding, the float types and the 64 MB budget."""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]


def _bench():
    sys.path.insert(0, str(ROOT))
    import bench
    return bench


def test_options_default_to_a_plain_run():
    bench = _bench()
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def _pipeline(Q, R, lens, M, qpp=True, weights=False, seed=1):
    """Host stand-in for bench.Pipeline after a step: ragged lists (lens [Q*R]), unions
    shorter than the query, the buffers' unwritten tails poisoned."""
    from qppfuse.engine import FuseOut
    rng = np.random.default_rng(seed)
    off = np.zeros(Q * R + 1, np.int64)
    off[1:] = np.cumsum(lens)
    E = int(off[-1])
    span = off[R::R] - off[:-R:R]
    uc = np.maximum(1, span - rng.integers(0, 3, Q)).astype(np.int32)
    ud = rng.integers(0, 2**32, E, dtype=np.uint64).astype(np.uint32)
    fused = rng.normal(size=(M, E))
    perm = np.zeros((M, E), np.uint16)
    valid = np.zeros(E, bool)
    for q in range(Q):
        b = off[q * R]
        valid[b:b + uc[q]] = True
        for m in range(M):
            perm[m, b:b + uc[q]] = rng.permutation(uc[q])
    ud[~valid] = 0xDEADBEEF
    fused[:, ~valid] = np.nan
    perm[:, ~valid] = 0xFFFF
    t = torch.from_numpy
    out = FuseOut(t(ud.view(np.int32)), t(uc), t(perm.view(np.int16)), t(fused), ["m"] * M)
    p = SimpleNamespace(
        Q=Q, R=R, out=out, methods=["combsum", "rrf", "wcombsum"][:M], q_begin=1000,
        args=SimpleNamespace(wl={"qpp": qpp}), off=t(off),
        micro=t(rng.integers(0, 1_000_001, E).astype(np.int32)),
        qraw=t(rng.normal(size=(Q * R, 13))), mm=t(rng.normal(size=2 * R * 13)),
        qmicro=t(rng.integers(0, 1_000_001, Q * R * 13)),
        w=t(rng.random(Q * R)) if weights else None)
    return p, off, uc, ud, fused, perm


def test_dump_sample_padding_and_types(tmp_path):
    bench = _bench()
    Q, R, M = 100, 3, 2
    lens = np.random.default_rng(0).integers(1, 9, Q * R)
    p, off, uc, ud, fused, perm = _pipeline(Q, R, lens, M, weights=True)
    shapes = bench.dump_outputs(p, tmp_path / "d")
    a = {f.stem: np.load(f) for f in (tmp_path / "d").iterdir()}
    assert set(a) == set(shapes) == {
        "union_count", "qpp_raw", "qpp_colminmax", "qpp_micro", "fusion_weights",
        "sample_queries", "sample_norm_micro", "sample_union_docid", "sample_fused", "sample_perm"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert all(list(a[k].shape) == s for k, s in shapes.items())
    assert np.array_equal(a["union_count"], uc)
    assert a["qpp_raw"].tobytes() == p.qraw.numpy().tobytes()
    assert np.array_equal(a["qpp_micro"].ravel(), p.qmicro.numpy())
    assert a["fusion_weights"].shape == (Q, R)
    sample = a["sample_queries"].astype(np.int64) - p.q_begin
    want = np.sort(np.random.default_rng(bench.SEED).choice(Q, bench.DUMP_SAMPLE_QUERIES,
                                                            replace=False))
    assert np.array_equal(sample, want)  # fixed by the seed alone
    n = a["sample_fused"].shape[2]
    assert n == (off[(sample + 1) * R] - off[sample * R]).max()
    for i, q in enumerate(sample):
        b, e, u = off[q * R], off[(q + 1) * R], uc[q]
        assert np.array_equal(a["sample_norm_micro"][i, :e - b], p.micro.numpy()[b:e])
        assert np.all(a["sample_norm_micro"][i, e - b:] == 0)
        assert np.array_equal(a["sample_union_docid"][i, :u], ud[b:b + u])
        assert np.all(a["sample_union_docid"][i, u:] == -1)
        assert a["sample_fused"][i, :, :u].tobytes() == fused[:, b:b + u].tobytes()
        assert np.all(a["sample_fused"][i, :, u:] == 0)  # never the unwritten tail
        assert np.array_equal(a["sample_perm"][i, :, :u], perm[:, b:b + u])
        assert np.all(a["sample_perm"][i, :, u:] == -1)


def test_dump_without_qpp_and_fewer_queries_than_the_sample(tmp_path):
    bench = _bench()
    p, *_ = _pipeline(5, 2, np.full(10, 4), 1, qpp=False)
    shapes = bench.dump_outputs(p, tmp_path)
    assert "qpp_raw" not in shapes and "fusion_weights" not in shapes
    assert shapes["sample_queries"] == [5] and shapes["sample_fused"] == [5, 1, 8]


def test_dump_keeps_to_the_budget(tmp_path, monkeypatch):
    """Long lists: fewer sampled queries, never more than the limit."""
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 200_000)
    Q, R, M = 80, 2, 3
    p, *_ = _pipeline(Q, R, np.full(Q * R, 50), M)
    shapes = bench.dump_outputs(p, tmp_path)
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= 200_000
    whole = 8 * (Q + Q * R * 13 * 2 + 2 * R * 13) + 4096  # with the .npy headers' share
    per_query = 100 * (4 + 8 + M * 12) + 8
    assert shapes["sample_queries"] == [(200_000 - whole) // per_query]
    assert 1 < shapes["sample_queries"][0] < bench.DUMP_SAMPLE_QUERIES
