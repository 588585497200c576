"""bench.py --dump-outputs without a GPU: the serving loop of the timed path driven against a stand-in engine that answers
in a seeded random order, so that each stream's progress through the window depends on that order as it depends on timing
on the device.  What is captured - every stream's reply to the last timed chunk - must not."""
import numpy as np
import pytest

import bench


class FakeBatch:
    """the calls serve() / serve_rest() make of a NativeStreamBatch; the chunk index travels in the PCM (column 0) and
    the reply of stream s to chunk k is a function of (s, k) alone"""

    def __init__(self, S, seed, lcap=12):
        self.S, self.lcap = S, lcap
        self.rng = np.random.default_rng(seed)
        self.inflight = {}
        self.answered = {}
        self.st = [type("St", (), {"n_steps_total": 0})() for _ in range(S)]
        self.stats = {"dec_steps": 0, "enc_calls": 0}

    @staticmethod
    def reply(s, k):
        n = 1 + (s + k) % 9
        return {"ids": np.arange(n) + 100 * s + k, "xpos": np.arange(n) + k, "len": n, "score": -0.5 * k - s / 7.0}

    def take_attn_counters(self):
        return {}

    @property
    def outstanding(self):
        return len(self.inflight)

    def submit_block(self, streams, pcm):
        for s, row in zip(streams, pcm):
            assert int(s) not in self.inflight
            self.inflight[int(s)] = int(row[0])

    def poll_ids(self, min_done=1, max_done=0):
        ready = list(self.inflight)
        n = min(len(ready), max(min_done, int(self.rng.integers(1, len(ready) + 1))))
        done = np.array(sorted(self.rng.choice(ready, n, replace=False)), dtype=np.int32)
        for s in done:
            self.answered[int(s)] = self.inflight.pop(int(s))
        return done, np.zeros(n, np.int32)

    def hypotheses_arrays(self, streams, nbest=None):
        n = len(streams)
        lmax = self.lcap if n > 4 else max(self.reply(int(s), self.answered[int(s)])["len"] for s in streams)
        ids = np.full((n, 1, lmax), 7, np.int32)           # (junk beyond a hypothesis' length: the dump zeroes it)
        xp = np.full((n, 1, lmax), 7, np.int32)
        lens = np.zeros((n, 1), np.int32)
        sc = np.zeros((n, 1))
        for i, s in enumerate(streams):
            r = self.reply(int(s), self.answered[int(s)])
            ids[i, 0, :r["len"]], xp[i, 0, :r["len"]], lens[i, 0], sc[i, 0] = r["ids"], r["xpos"], r["len"], r["score"]
        return {"ids": ids, "xpos": xp, "lens": lens, "n_hyps": np.ones(n, np.int32), "score": sc}


def _dump(tmp_path, seed, S=16, preroll=3, warmup=2, steps=5, group=3):
    chunks = preroll + warmup + steps + bench.SERVED_SPARE
    a3 = np.zeros((S, chunks, 2), np.float32)
    a3[:, :, 0] = np.arange(chunks)
    sb = FakeBatch(S, seed)
    cap = bench.ReplyCapture(S, preroll + warmup + steps - 1)
    nxt = np.full(S, preroll, np.int64)
    bench.serve(sb, a3, nxt, warmup, group, capture=cap)
    res = bench.serve(sb, a3, nxt, steps, group, capture=cap)
    spread = res["chunks_per_stream_min_max"]
    bench.serve_rest(sb, a3, nxt, group, cap)
    assert not len(cap.missing())
    files = bench.write_outputs(str(tmp_path / str(seed)), cap.rows)
    return {f[:-len(".npy")]: np.load(tmp_path / str(seed) / f) for f in files}, spread, cap.k


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(bench.torch.cuda, "synchronize", lambda *a, **k: None)


def test_dump_is_the_reply_to_the_last_timed_chunk_whatever_the_order(tmp_path, no_device):
    runs = [_dump(tmp_path, seed) for seed in (1, 2, 3)]
    assert any(lo != hi for _, (lo, hi), _ in runs)        # the order did move the streams apart in the window
    first, _, k = runs[0]
    assert sorted(first) == ["ids", "lens", "n_hyps", "score", "stream", "xpos"]
    for d, _, _ in runs[1:]:
        for f in first:
            assert d[f].dtype == first[f].dtype and np.array_equal(d[f], first[f]), f
    S = len(first["stream"])
    for s in range(S):
        r = FakeBatch.reply(s, k)
        n = r["len"]
        assert first["lens"][s, 0] == n and first["score"][s, 0] == r["score"]
        assert np.array_equal(first["ids"][s, 0, :n], r["ids"]) and not first["ids"][s, 0, n:].any()
        assert np.array_equal(first["xpos"][s, 0, :n], r["xpos"]) and not first["xpos"][s, 0, n:].any()
    assert first["ids"].shape[-1] == max(FakeBatch.reply(s, k)["len"] for s in range(S))
    for f, a in first.items():
        assert a.dtype == (np.float64 if f == "score" else np.float32), f


def test_dump_stays_under_its_cap_with_a_fixed_sample(tmp_path):
    rows = [{"ids": np.full((1, 50), s, np.int32), "lens": np.array([50], np.int32), "score": np.array([float(s)])}
            for s in range(40)]
    bench.write_outputs(str(tmp_path / "a"), rows, cap_bytes=4000)
    bench.write_outputs(str(tmp_path / "b"), rows, cap_bytes=4000)
    total = sum((tmp_path / "a" / f).stat().st_size for f in ("ids.npy", "lens.npy", "score.npy", "stream.npy"))
    assert total <= 4000 + 4 * 128                                     # (+ the .npy headers)
    keep = np.load(tmp_path / "a" / "stream.npy")
    assert 0 < len(keep) < 40 and np.array_equal(keep, np.load(tmp_path / "b" / "stream.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "score.npy")[:, 0], keep)
