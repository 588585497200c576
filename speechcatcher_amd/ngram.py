"""Backoff n-gram language models for the CTC prefix beam (csrc/lm_blob.h, sc_lm_create, sc_ctc_beam_lm).

A model is a plain dict {n-gram tuple of token ids: (logp, backoff)}, natural logs, closed under prefixes (the context
of every n-gram is itself an n-gram of the dict).  ``pack`` turns it into the blob the library takes - a backoff
automaton:
    state      a context the model holds (an n-gram shorter than the order); state 0 is the empty context.  Per state
               ``backoff`` (float64) and ``bo_state``: the state of the longest proper suffix of the context that the
               model holds (the context without its oldest token when the model is closed under suffixes; a context the
               model does not hold has backoff 0, so skipping it changes no sum).
    arc        (state, token) -> (logp float64, next): next = the state of the longest suffix of context + token that
               the model holds.  State 0's arcs are a dense [V] array (a token without a unigram gets FLOOR and next 0);
               all others live in ONE open-addressing hash table, key (state << 32) | token, linear probing.
    score(s, c):  acc = 0.0;  while s != 0 and (s, c) has no arc: acc = acc + backoff[s]; s = bo_state[s]
                  -> (acc + logp[s, c], next[s, c])            float64 additions in exactly this order

The blob (little endian; include/scasr.h, "language model blob"): 8 int32 words MAGIC, VERSION, V, order, n_states,
n_arcs, n_slots, start_state; float64 backoff[n_states]; int32 bo_state[n_states] (padded to 8 bytes); float64
root_logp[V]; int32 root_next[V] (padded); n_slots slots of 24 bytes (uint64 key, float64 logp, int32 next, int32 0),
n_slots a power of two >= 2, an unused slot has the key EMPTY and is otherwise zero.  The home slot of a key is
(key * HASH_MUL mod 2^64) >> (64 - log2 n_slots).

    python -m speechcatcher_amd.ngram [--alias WORD=TOKEN ...] in.arpa tokens.txt out.sclm

``--alias WORD=TOKEN`` (may be repeated): the ARPA word WORD stands for the entry TOKEN of the token list.  ESPnet token
lists have ONE <sos/eos> entry where ARPA files have <s> and </s>: ``--alias "<s>=<sos/eos>" --alias "</s>=<sos/eos>"``.
When two ARPA words map to one id, the id's unigram takes its logp from </s> and its backoff from <s>: the id is predicted
only as an end and conditions only as a start.  The start state (``bos``) and the id printed as "eos" follow the aliases.
"""
import math
import struct
import sys
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

MAGIC = 0x4D4C4353          # "SCLM"
VERSION = 1
MAX_ORDER = 5               # SC_LM_MAX_ORDER
EMPTY = (1 << 64) - 1
HASH_MUL = 0x9E3779B97F4A7C15
SLOT_BYTES = 24
HEADER_WORDS = 8
LN10 = math.log(10.0)
FLOOR = -99.0 * LN10        # ARPA's "-99": the log probability of what a model does not hold
SLOT_DT = np.dtype([("key", "<u8"), ("logp", "<f8"), ("next", "<i4"), ("pad", "<i4")])

Model = Dict[Tuple[int, ...], Tuple[float, float]]


def home(key: int, bits: int) -> int:
    return ((key * HASH_MUL) & EMPTY) >> (64 - bits)


def _pad8(n: int) -> int:
    return (n + 7) & ~7


def order_of(model: Model) -> int:
    return max((len(g) for g in model), default=1)


def pack(model: Model, V: int, order: Optional[int] = None, bos: Optional[int] = None, load: float = 0.5) -> bytes:
    """the blob of ``model`` over the token ids [0, V).  ``order``: the model's (default: its longest n-gram);
    ``bos``: the id of the sentence start - the automaton starts in the state of the context (bos,) when the model
    holds it; ``load``: the hash table holds at most this share of used slots (0 < load < 1)."""
    order = order_of(model) if order is None else int(order)
    if not 1 <= order <= MAX_ORDER:
        raise ValueError(f"order {order} outside [1, {MAX_ORDER}]")
    if V < 1 or not 0.0 < load < 1.0:
        raise ValueError("V >= 1 and 0 < load < 1 are required")
    for g, (lp, bo) in model.items():
        if not 1 <= len(g) <= order or any(not 0 <= int(t) < V for t in g):
            raise ValueError(f"n-gram {g}: length outside [1, {order}] or a token outside [0, {V})")
        if not (math.isfinite(lp) and math.isfinite(bo)):
            raise ValueError(f"n-gram {g}: logp / backoff must be finite, got ({lp}, {bo})")
        if len(g) > 1 and g[:-1] not in model:
            raise ValueError(f"n-gram {g}: its context {g[:-1]} is not in the model (not closed under prefixes)")
    ctxs = sorted((g for g in model if len(g) < order), key=lambda g: (len(g), g))
    sid = {(): 0}
    for g in ctxs:
        sid[g] = len(sid)

    def held(g):   # the state of the longest suffix of g that the model holds as a context
        g = g[max(0, len(g) - (order - 1)):] if order > 1 else ()
        while g not in sid:
            g = g[1:]
        return sid[g]

    n_states = len(sid)
    backoff = np.zeros(n_states, np.float64)
    bo_state = np.zeros(n_states, np.int32)
    for g, s in sid.items():
        if s:
            backoff[s] = model[g][1]
            bo_state[s] = held(g[1:])
    root_logp = np.full(V, FLOOR, np.float64)
    root_next = np.zeros(V, np.int32)
    arcs = []
    for g, (lp, _) in model.items():
        if len(g) == 1:
            root_logp[g[0]] = lp
            root_next[g[0]] = held(g)
        else:
            arcs.append(((sid[g[:-1]] << 32) | int(g[-1]), float(lp), held(g)))
    bits = 1
    while (1 << bits) * load < len(arcs):
        bits += 1
    n_slots = 1 << bits
    slots = np.zeros(n_slots, SLOT_DT)
    slots["key"] = EMPTY
    for key, lp, nxt in sorted(arcs):
        k = home(key, bits)
        while slots[k]["key"] != EMPTY:
            k = (k + 1) & (n_slots - 1)
        slots[k] = (key, lp, nxt, 0)
    start = sid.get((int(bos),), 0) if bos is not None and order > 1 else 0
    head = struct.pack("<8i", MAGIC, VERSION, V, order, n_states, len(arcs), n_slots, start)

    def sect(a):
        b = a.tobytes()
        return b + b"\0" * (_pad8(len(b)) - len(b))

    return head + sect(backoff) + sect(bo_state) + sect(root_logp) + sect(root_next) + slots.tobytes()


class Blob:
    """numpy views of a packed blob and the automaton's ``score`` on them (what the device code does)"""

    def __init__(self, blob: bytes):
        w = struct.unpack_from("<8i", blob, 0)
        if w[0] != MAGIC or w[1] != VERSION:
            raise ValueError("not a language model blob of this version")
        _, _, self.V, self.order, self.n_states, self.n_arcs, self.n_slots, self.start_state = w
        off = 4 * HEADER_WORDS
        self.backoff = np.frombuffer(blob, "<f8", self.n_states, off)
        off += 8 * self.n_states
        self.bo_state = np.frombuffer(blob, "<i4", self.n_states, off)
        off += _pad8(4 * self.n_states)
        self.root_logp = np.frombuffer(blob, "<f8", self.V, off)
        off += 8 * self.V
        self.root_next = np.frombuffer(blob, "<i4", self.V, off)
        off += _pad8(4 * self.V)
        self.slots = np.frombuffer(blob, SLOT_DT, self.n_slots, off)
        if off + SLOT_BYTES * self.n_slots != len(blob):
            raise ValueError("the blob's size does not match its header")
        self.bits = self.n_slots.bit_length() - 1
        self._keys = self.slots["key"].tolist()
        self.longest_probe = 0

    def find(self, s: int, c: int):
        """the slot of arc (s, c), s != 0; None when there is none"""
        key = (s << 32) | c
        k, steps = home(key, self.bits), 1
        while self._keys[k] != EMPTY:
            if self._keys[k] == key:
                self.longest_probe = max(self.longest_probe, steps)
                return self.slots[k]
            k, steps = (k + 1) & (self.n_slots - 1), steps + 1
        self.longest_probe = max(self.longest_probe, steps)
        return None

    def score(self, s: int, c: int):
        acc = 0.0
        while s != 0:
            slot = self.find(s, c)
            if slot is not None:
                return float(acc + float(slot["logp"])), int(slot["next"])
            acc = float(acc + float(self.backoff[s]))
            s = int(self.bo_state[s])
        return float(acc + float(self.root_logp[c])), int(self.root_next[c])


def word_ids(tokens: Sequence[str], alias: Optional[Dict[str, str]] = None) -> Dict[str, int]:
    """ARPA word -> token id: the token list's entries, and every alias WORD -> the id of its TOKEN"""
    ids = {t: i for i, t in enumerate(tokens)}
    for word, tok in (alias or {}).items():
        if tok not in ids:
            raise ValueError(f"alias {word}={tok}: '{tok}' is not in the token list")
        ids[word] = ids[tok]
    return ids


def parse_arpa(text: str, tokens: Sequence[str], alias: Optional[Dict[str, str]] = None) -> Tuple[Model, int]:
    """ARPA text -> (model, order): log10 -> ln, words -> ids through ``tokens`` (an n-gram with a word that is not
    among them is left out - with it every n-gram that extends it, so the model stays closed under prefixes); "-99"
    becomes FLOOR; an n-gram without a backoff column has backoff 0.  ``alias``: {ARPA word: entry of ``tokens``} (the
    module's doc).  Two unigrams on one id merge when one of them is <s>: logp from the other word (</s>), backoff from
    <s>; any other pair of words on one id is an error.  Of two longer n-grams on the same ids the first is kept."""
    ids = word_ids(tokens, alias)
    model: Model = {}
    first: Dict[int, str] = {}   # id -> the word of its first unigram
    n, order = 0, 0
    for line in text.splitlines():
        line = line.strip()
        if not line or line == "\\data\\" or line.startswith("ngram "):
            continue
        if line == "\\end\\":
            break
        if line.startswith("\\") and line.endswith("-grams:"):
            n = int(line[1:line.index("-")])
            order = max(order, n)
            continue
        if n == 0:
            continue
        col = line.split()
        if len(col) not in (n + 1, n + 2):
            raise ValueError(f"ARPA: {n}-gram line with {len(col)} columns: {line!r}")
        lp10, words = float(col[0]), col[1:n + 1]
        bo10 = float(col[n + 1]) if len(col) == n + 2 else 0.0
        if not (math.isfinite(lp10) and math.isfinite(bo10)):
            raise ValueError(f"ARPA: infinite or NaN value: {line!r}")
        if any(w not in ids for w in words):
            continue
        g = tuple(ids[w] for w in words)
        if len(g) > 1 and g[:-1] not in model:
            continue
        if g in model:
            if n > 1:
                continue
            a, b = first[g[0]], words[0]
            if "<s>" not in (a, b) or a == b:
                raise ValueError(f"ARPA: the words {a!r} and {b!r} map to one token id and neither is <s>")
            other, start = (model[g], (lp10 * LN10, bo10 * LN10)) if b == "<s>" else ((lp10 * LN10, bo10 * LN10), model[g])
            model[g] = (other[0], start[1])   # predicted as an end, conditions as a start
            continue
        if n == 1:
            first[g[0]] = words[0]
        model[g] = (lp10 * LN10, bo10 * LN10)
    if order == 0:
        raise ValueError("ARPA: no n-gram section")
    return model, order


def to_arpa(model: Model, tokens: Sequence[str], order: Optional[int] = None) -> str:
    """the model as ARPA text (17 significant digits: parse_arpa gives the values back to the last few ulp of the
    log10 <-> ln conversion)"""
    order = order_of(model) if order is None else order
    by = [[g for g in sorted(model) if len(g) == n] for n in range(1, order + 1)]
    out = ["\\data\\"] + [f"ngram {n + 1}={len(gs)}" for n, gs in enumerate(by)] + [""]
    for n, gs in enumerate(by):
        out.append(f"\\{n + 1}-grams:")
        for g in gs:
            lp, bo = model[g]
            tail = f"\t{bo / LN10!r}" if n + 1 < order else ""
            out.append(f"{lp / LN10!r}\t" + " ".join(tokens[t] for t in g) + tail)
        out.append("")
    return "\n".join(out + ["\\end\\", ""])


def load(source) -> bytes:
    """``source`` as the scheduler and the CLI take it: the blob itself (bytes) or the path of a packed file"""
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source)
    with open(source, "rb") as fh:
        return fh.read()


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    alias: Dict[str, str] = {}
    while "--alias" in argv:
        k = argv.index("--alias")
        word, sep, tok = (argv[k + 1] if k + 1 < len(argv) else "").partition("=")
        if not (word and sep and tok):
            print("--alias takes WORD=TOKEN", file=sys.stderr)
            return 2
        alias[word] = tok
        del argv[k:k + 2]
    if len(argv) != 3:
        print("usage: python -m speechcatcher_amd.ngram [--alias WORD=TOKEN ...] in.arpa tokens.txt out.sclm", file=sys.stderr)
        return 2
    with open(argv[1], encoding="utf-8") as fh:
        tokens = [line.rstrip("\n").split(" ")[0] for line in fh if line.strip()]
    with open(argv[0], encoding="utf-8") as fh:
        model, order = parse_arpa(fh.read(), tokens, alias)
    ids = word_ids(tokens, alias)
    bos = ids.get("<s>")
    blob = pack(model, len(tokens), order, bos=bos)
    with open(argv[2], "wb") as fh:
        fh.write(blob)
    b = Blob(blob)
    print(f"{argv[2]}: order {b.order}, V {b.V}, {b.n_states} states, {b.n_arcs} arcs in {b.n_slots} slots, "
          f"{len(blob)} bytes" + (f", bos {bos}, eos {ids.get('</s>')}" if alias else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
