"""The validator of language model blobs (speechcatcher_amd/csrc/lm_blob.h) without a GPU: tests/host/lm_blob_check.cpp
- a stand-alone program that includes nothing but that header - is compiled with the host compiler, with the address
and undefined-behaviour sanitizers when the compiler links them, and handed one good blob and a list of corrupted ones,
each in a heap block of exactly its size: it accepts the good one and rejects every other without reading out of bounds."""
import shutil
import struct
import subprocess

import numpy as np
import pytest

import ngram_ref as NR
from conftest import ROOT
from speechcatcher_amd import ngram

V = 6


def _good():
    rng = np.random.default_rng(5)
    sents = [[int(t) for t in rng.integers(1, V, int(rng.integers(2, 9)))] for _ in range(40)]
    return ngram.pack(NR.estimate(sents, V, 3), V, 3)


def _corrupted(good: bytes):
    b = ngram.Blob(good)
    off_bo = 32 + 8 * b.n_states
    off_rl = off_bo + ngram._pad8(4 * b.n_states)
    off_rn = off_rl + 8 * V
    off_sl = off_rn + ngram._pad8(4 * V)
    used = [k for k in range(b.n_slots) if int(b.slots[k]["key"]) != ngram.EMPTY]
    free = [k for k in range(b.n_slots) if int(b.slots[k]["key"]) == ngram.EMPTY]

    def patch(off, fmt, *vals, src=good):
        m = bytearray(src)
        struct.pack_into(fmt, m, off, *vals)
        return bytes(m)

    slot = lambda k: off_sl + 24 * k   # noqa: E731
    out = {
        "empty": b"",
        "truncated header": good[:20],
        "truncated": good[:-8],
        "one byte short": good[:-1],
        "trailing bytes": good + b"\0" * 8,
        "magic": patch(0, "<i", 0x12345678),
        "version": patch(4, "<i", 2),
        "order 6": patch(12, "<i", 6),
        "huge n_states": patch(16, "<i", 0x7fffffff),
        "negative V": patch(8, "<i", -1),
        "slots no power of two": patch(24, "<i", b.n_slots - 1),
        "start_state out of range": patch(28, "<i", b.n_states),
        "next out of range": patch(slot(used[0]) + 16, "<i", b.n_states),
        "next negative": patch(slot(used[1]) + 16, "<i", -1),
        "root next out of range": patch(off_rn + 4, "<i", b.n_states + 3),
        "bo_state out of range": patch(off_bo + 4, "<i", b.n_states),
        "bo_state cycle": patch(off_bo + 4, "<i", 2, src=patch(off_bo + 8, "<i", 1)),
        "bo_state self loop": patch(off_bo + 4 * 3, "<i", 3),
        "NaN logp": patch(slot(used[2]) + 8, "<d", float("nan")),
        "inf backoff": patch(32 + 8, "<d", float("-inf")),
        "NaN unigram": patch(off_rl, "<d", float("nan")),
        "key state out of range": patch(slot(used[0]), "<Q", (b.n_states << 32) | 1),
        "key token out of range": patch(slot(used[0]), "<Q", (1 << 32) | V),
    }
    # the key of one used slot a second time, in the unused slot that ends its probe run
    k = used[0]
    end = k
    while int(b.slots[end]["key"]) != ngram.EMPTY:
        end = (end + 1) % b.n_slots
    dup = patch(slot(end), "<Qdii", int(b.slots[k]["key"]), -1.0, 0, 0)
    out["duplicate key"] = patch(20, "<i", b.n_arcs + 1, src=dup)
    # every slot used: no probe run ends
    full = bytearray(good)
    for i, f in enumerate(free):
        struct.pack_into("<Qdii", full, slot(f), (1 << 32) | (V + 1 + i), -1.0, 0, 0)
    out["full probe run"] = patch(20, "<i", b.n_slots, src=bytes(full))
    out["full probe run, honest count"] = patch(20, "<i", b.n_slots - 1, src=bytes(full))
    # a key moved out of its probe run: the slot it leaves unused ends the run before the slot it moves to
    moved = bytearray(good)
    moved[slot(free[-1]):slot(free[-1]) + 24] = good[slot(k):slot(k) + 24]
    struct.pack_into("<Qdii", moved, slot(k), ngram.EMPTY, 0.0, 0, 0)
    out["unreachable key"] = bytes(moved)
    return out


def test_the_validator_accepts_a_good_blob_and_rejects_every_corrupted_one(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "lm_blob_check"
    base = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", str(ROOT / "tests" / "host" / "lm_blob_check.cpp"), "-o",
            str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    sanitized = subprocess.run(base + san, capture_output=True).returncode == 0
    if not sanitized:   # (a compiler that does not link the sanitizers: the validator is still checked, unsanitized)
        subprocess.run(base, check=True)
    good = _good()
    cases = _corrupted(good)
    for need in ("truncated", "next out of range", "bo_state cycle", "NaN logp", "duplicate key", "full probe run"):
        assert need in cases
    names = ["good"] + list(cases)
    for name, blob in zip(names, [good] + list(cases.values())):
        (tmp_path / f"{names.index(name)}.sclm").write_bytes(blob)
    res = subprocess.run([str(exe)] + [str(tmp_path / f"{i}.sclm") for i in range(len(names))], capture_output=True,
                         text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr            # (a sanitizer report ends the program with an error)
    lines = res.stdout.splitlines()
    assert len(lines) == len(names), res.stdout
    b = ngram.Blob(good)
    assert lines[0] == f"ok {V} 3 {b.n_states} {b.n_arcs} {b.n_slots} 0", lines[0]
    for name, line in zip(names[1:], lines[1:]):
        assert line.startswith("bad: "), (name, line)
    print(f"\nlm_blob_check: sanitizers {'on' if sanitized else 'NOT linked by this compiler'}; "
          + "; ".join(f"{n}: {ln[5:]}" for n, ln in zip(names[1:], lines[1:])))
