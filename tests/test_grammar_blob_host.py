"""The validator of grammar blobs (speechcatcher_amd/csrc/grammar_blob.h) without a GPU: tests/host/grammar_blob_check.cpp
- a stand-alone program that includes nothing but that header - is compiled with the host compiler, with the address and
undefined-behaviour sanitizers when the compiler links them, and handed one good blob and one corrupted blob per rule
of the validator, each in a heap block of exactly its size: it accepts the good one and rejects every other without
reading out of bounds."""
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from speechcatcher_amd import grammar

V, BLANK = 9, 2


def _good():
    rng = np.random.default_rng(5)
    toks = [t for t in range(V) if t != BLANK]
    return grammar.compile([[int(rng.choice(toks)) for _ in range(int(rng.integers(1, 5)))] for _ in range(12)], V, BLANK)


def _corrupted(good: bytes):
    g = grammar.Grammar(good)
    ns, na = g.n_states, g.n_arcs
    off_off = 32
    off_tok = off_off + grammar._pad8(4 * (ns + 1))
    off_nxt = off_tok + grammar._pad8(4 * na)
    off_acc = off_nxt + grammar._pad8(4 * na)
    wide = next(s for s in range(ns) if g.arc_off[s + 1] - g.arc_off[s] >= 2)   # a state with two arcs or more
    a = int(g.arc_off[wide])

    def patch(off, fmt, *vals, src=good):
        m = bytearray(src)
        struct.pack_into(fmt, m, off, *vals)
        return bytes(m)

    return {
        "empty": b"",
        "truncated header": good[:20],
        "truncated": good[:-8],
        "one byte short": good[:-1],
        "trailing bytes": good + b"\0" * 8,
        "magic": patch(0, "<i", 0x12345678),
        "version": patch(4, "<i", 2),
        "V zero": patch(8, "<i", 0),
        "negative V": patch(8, "<i", -1),
        "blank out of range": patch(12, "<i", V),
        "blank negative": patch(12, "<i", -1),
        "no state": patch(16, "<i", 0),
        "huge n_states": patch(16, "<i", 0x7fffffff),
        "n_states over the limit": patch(16, "<i", (1 << 20) + 1),
        "negative n_arcs": patch(20, "<i", -1),
        "n_arcs over the limit": patch(20, "<i", (1 << 24) + 1),
        "n_arcs one more": patch(20, "<i", na + 1),
        "start_state out of range": patch(24, "<i", ns),
        "start_state negative": patch(24, "<i", -1),
        "reserved word": patch(28, "<i", 1),
        "arc_off[0] not 0": patch(off_off, "<i", 1),
        "arc_off end not n_arcs": patch(off_off + 4 * ns, "<i", na - 1),
        "arc_off not monotone": patch(off_off + 4 * (wide + 1), "<i", a - 1 if a > 0 else na + 5),
        "arc_off beyond n_arcs": patch(off_off + 4 * 1, "<i", na + 100),
        "arc_off negative": patch(off_off + 4 * 1, "<i", -4),
        "tokens descending": patch(off_tok + 4 * a, "<ii", int(g.arc_tok[a + 1]), int(g.arc_tok[a])),
        "token twice": patch(off_tok + 4 * (a + 1), "<i", int(g.arc_tok[a])),
        "token out of range": patch(off_tok + 4 * (int(g.arc_off[wide + 1]) - 1), "<i", V),
        "token negative": patch(off_tok + 4 * a, "<i", -1),
        "token is the blank": patch(12, "<i", int(g.arc_tok[a])),
        "next out of range": patch(off_nxt + 4 * (na - 1), "<i", ns),
        "next negative": patch(off_nxt, "<i", -1),
        "accept flag 2": patch(off_acc + 4 * (ns - 1), "<i", 2),
        "accept flag negative": patch(off_acc, "<i", -1),
    }


def test_the_validator_accepts_a_good_blob_and_rejects_every_corrupted_one(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "grammar_blob_check"
    base = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", str(ROOT / "tests" / "host" / "grammar_blob_check.cpp"),
            "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    sanitized = subprocess.run(base + san, capture_output=True).returncode == 0
    if not sanitized:   # (a compiler that does not link the sanitizers: the validator is still checked, unsanitized)
        subprocess.run(base, check=True)
    good = _good()
    cases = _corrupted(good)
    blobs = {"good": good, "free": grammar.free(V, BLANK), "no arcs at all": grammar.pack(V, BLANK, [[]], [0]), **cases}
    names = list(blobs)
    for i, name in enumerate(names):
        (tmp_path / f"{i}.scgr").write_bytes(blobs[name])
    res = subprocess.run([str(exe)] + [str(tmp_path / f"{i}.scgr") for i in range(len(names))], capture_output=True,
                         text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr            # (a sanitizer report ends the program with an error)
    lines = res.stdout.splitlines()
    assert len(lines) == len(names), res.stdout
    g = grammar.Grammar(good)
    assert lines[0] == f"ok {V} {BLANK} {g.n_states} {g.n_arcs} 0", lines[0]
    assert lines[1] == f"ok {V} {BLANK} 1 {V - 1} 0" and lines[2] == f"ok {V} {BLANK} 1 0 0", lines[1:3]
    for name, line in zip(names[3:], lines[3:]):
        assert line.startswith("bad: "), (name, line)
    reasons = {line[5:] for line in lines[3:]}
    assert len(reasons) >= 12, reasons                               # every rule of the validator has spoken
    print(f"\ngrammar_blob_check: sanitizers {'on' if sanitized else 'NOT linked by this compiler'}; "
          + "; ".join(f"{n}: {ln[5:]}" for n, ln in zip(names[3:], lines[3:])))
