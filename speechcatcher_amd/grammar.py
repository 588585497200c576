"""Grammars for the CTC prefix beam: "answer only from this list" (csrc/grammar_blob.h, sc_grammar_create,
sc_ctc_beam_grammar).

A grammar is a deterministic finite automaton over the token ids [0, V); the blank is never a label.  State g has the
out-arcs (token -> next), strictly ascending by token, and an accept flag; there is one start state.  ``compile`` builds
it from phrases given as token-id sequences: a trie of the phrases - with ``loop`` phrases may follow each other, so an
accepting state also offers the start state's arcs -, made deterministic by subset construction (a phrase that is a prefix
of another makes the plain trie ambiguous under ``loop``).  States are numbered in breadth-first order from the start
state, arcs by ascending token: the same phrases give the same bytes, in whatever order they are listed.

The blob (little endian; include/scasr.h, "grammar-constrained CTC prefix beam"): 8 int32 words MAGIC, VERSION, V, blank,
n_states, n_arcs, start_state, 0; int32 arc_off[n_states + 1]; int32 arc_tok[n_arcs]; int32 arc_next[n_arcs]; int32
accept[n_states] - every array padded to a multiple of 8 bytes.

    python -m speechcatcher_amd.grammar phrases.txt tokens.txt out.scgr

packs one phrase per line, tokenised by ``spotting.phrase_ids``.
"""
import struct
import sys
from typing import Iterable, List, Sequence

import numpy as np

MAGIC = 0x52474353          # "SCGR"
VERSION = 1
MAX_STATES = 1 << 20        # SC_GRAMMAR_MAX_STATES
MAX_ARCS = 1 << 24          # SC_GRAMMAR_MAX_ARCS
HEADER_WORDS = 8


def _pad8(n: int) -> int:
    return (n + 7) & ~7


def _sect(a: np.ndarray) -> bytes:
    b = a.astype("<i4").tobytes()
    return b + b"\0" * (_pad8(len(b)) - len(b))


def pack(V: int, blank: int, arcs: Sequence[Sequence[tuple]], accept: Sequence[int], start: int = 0) -> bytes:
    """the blob of an automaton given state by state: arcs[g] = [(token, next), ...] ascending by token"""
    off = np.cumsum([0] + [len(a) for a in arcs])
    tok = np.array([t for a in arcs for t, _ in a], np.int32)
    nxt = np.array([n for a in arcs for _, n in a], np.int32)
    head = struct.pack("<8i", MAGIC, VERSION, V, blank, len(arcs), len(tok), start, 0)
    return head + _sect(off) + _sect(tok) + _sect(nxt) + _sect(np.asarray(accept, np.int32))


def compile(phrases: Iterable[Sequence[int]], V: int, blank: int, loop: bool = True) -> bytes:   # noqa: A001
    """phrases (token-id sequences) -> the blob of the grammar that accepts exactly them - with ``loop``: them and their
    concatenations.  ValueError for an empty phrase list or phrase, a label outside [0, V) or equal to the blank, and a
    result of more than 2^20 states or 2^24 arcs."""
    V, blank = int(V), int(blank)
    if V < 1 or not 0 <= blank < V:
        raise ValueError(f"V >= 1 and a blank in [0, V) are required, got V = {V}, blank = {blank}")
    phrases = sorted({tuple(int(t) for t in ph) for ph in phrases})
    if not phrases:
        raise ValueError("a grammar needs at least one phrase")
    # the trie: node 0 is the root
    child: List[dict] = [{}]
    final = [False]
    for ph in phrases:
        if not ph:
            raise ValueError("an empty phrase")
        at = 0
        for t in ph:
            if not 0 <= t < V or t == blank:
                raise ValueError(f"phrase {list(ph)}: label {t} outside [0, {V}) or equal to the blank {blank}")
            if t not in child[at]:
                child[at][t] = len(child)
                child.append({})
                final.append(False)
            at = child[at][t]
        final[at] = True
    # subset construction, breadth first; a set that holds an accepting node offers the root's arcs too
    start = frozenset([0])
    ids = {start: 0}
    order = [start]
    arcs, accept, n_arcs = [], [], 0
    k = 0
    while k < len(order):
        S = order[k]
        k += 1
        acc = any(final[n] for n in S)
        out: dict = {}
        for n in sorted(S | ({0} if loop and acc else set())):
            for t, m in child[n].items():
                out.setdefault(t, set()).add(m)
        row = []
        for t in sorted(out):
            T = frozenset(out[t])
            if T not in ids:
                ids[T] = len(order)
                order.append(T)
                if len(order) > MAX_STATES:
                    raise ValueError(f"the grammar has more than {MAX_STATES} states")
            row.append((t, ids[T]))
        n_arcs += len(row)
        if n_arcs > MAX_ARCS:
            raise ValueError(f"the grammar has more than {MAX_ARCS} arcs")
        arcs.append(row)
        accept.append(1 if acc else 0)
    return pack(V, blank, arcs, accept, 0)


def free(V: int, blank: int) -> bytes:
    """the grammar that forbids nothing: one accepting state with a self-loop on every non-blank token"""
    return pack(V, blank, [[(t, 0) for t in range(V) if t != blank]], [1], 0)


class Grammar:
    """numpy views of a blob and the automaton's walk on them (what the device code and the library's host copy do)"""

    def __init__(self, blob: bytes):
        blob = bytes(blob)
        if len(blob) < 4 * HEADER_WORDS:
            raise ValueError("shorter than a grammar blob's header")
        w = struct.unpack_from("<8i", blob, 0)
        if w[0] != MAGIC or w[1] != VERSION:
            raise ValueError("not a grammar blob of this version")
        _, _, self.V, self.blank, self.n_states, self.n_arcs, self.start_state, _ = w
        if self.n_states < 1 or self.n_arcs < 0:
            raise ValueError("a grammar blob with bad counts")
        off = 4 * HEADER_WORDS
        sizes = (self.n_states + 1, self.n_arcs, self.n_arcs, self.n_states)
        if off + sum(_pad8(4 * n) for n in sizes) != len(blob):
            raise ValueError("the blob's size does not match its header")
        views = []
        for n in sizes:
            views.append(np.frombuffer(blob, "<i4", n, off))
            off += _pad8(4 * n)
        self.arc_off, self.arc_tok, self.arc_next, self.accept = views
        self.blob = blob

    def arcs(self, state: int):
        """[(token, next)] of a state, ascending by token"""
        a, b = int(self.arc_off[state]), int(self.arc_off[state + 1])
        return list(zip(self.arc_tok[a:b].tolist(), self.arc_next[a:b].tolist()))

    def step(self, state: int, token: int) -> int:
        """the next state, -1 when the state has no arc with that token"""
        if not 0 <= state < self.n_states:
            return -1
        a, b = int(self.arc_off[state]), int(self.arc_off[state + 1])
        k = a + int(np.searchsorted(self.arc_tok[a:b], token))
        return int(self.arc_next[k]) if k < b and int(self.arc_tok[k]) == token else -1

    def accepts(self, state: int) -> bool:
        return 0 <= state < self.n_states and bool(self.accept[state])

    def walk(self, ids: Sequence[int], state: int = None) -> int:
        """the state after ``ids`` from ``state`` (default: the start state), -1 when the walk leaves the grammar"""
        s = self.start_state if state is None else state
        for t in ids:
            s = self.step(s, int(t))
            if s < 0:
                return -1
        return s


def load(source) -> bytes:
    """``source`` as the scheduler and the CLI take it: the blob itself (bytes) or the path of a compiled file"""
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source)
    with open(source, "rb") as fh:
        return fh.read()


def from_text(lines: Iterable[str], tokens: Sequence[str], blank: int = 0, loop: bool = True) -> bytes:
    """one phrase per non-empty line, tokenised by spotting.phrase_ids"""
    from .spotting import phrase_ids
    return compile([phrase_ids(ln, tokens) for ln in (ln.strip() for ln in lines) if ln], len(tokens), blank, loop)


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    loop = True
    if "--no-loop" in argv:
        argv.remove("--no-loop")
        loop = False
    if len(argv) != 3:
        print("usage: python -m speechcatcher_amd.grammar [--no-loop] phrases.txt tokens.txt out.scgr", file=sys.stderr)
        return 2
    with open(argv[1], encoding="utf-8") as fh:
        tokens = [line.rstrip("\n").split(" ")[0] for line in fh if line.strip()]
    with open(argv[0], encoding="utf-8") as fh:
        blob = from_text(fh, tokens, 0, loop)
    with open(argv[2], "wb") as fh:
        fh.write(blob)
    g = Grammar(blob)
    print(f"{argv[2]}: V {g.V}, {g.n_states} states, {g.n_arcs} arcs, widest state "
          f"{int(np.diff(g.arc_off).max())} arcs, {len(blob)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
