"""The structs of the grammar-constrained beam (include/scasr.h: sc_beam_gr_t, sc_ctc_beam_gr_job, sc_grammar_header,
sc_grammar_view) against their ctypes mirrors in speechcatcher_amd/_abi.py and against the blob
speechcatcher_amd/grammar.py compiles: the C compiler's sizes and field offsets, the constants, and the argument errors
that return before any launch or allocation (no GPU needed)."""
import ctypes
import re
import shutil
import struct
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_struct_layouts_match_ctypes_and_the_compiler_of_grammars(tmp_path):
    from speechcatcher_amd import _abi, grammar
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    structs = {"sc_beam_gr_t": _abi.BeamGr, "sc_ctc_beam_gr_job": _abi.BeamGrJob, "sc_grammar_header": _abi.GrammarHeader,
               "sc_grammar_view": _abi.GrammarView, "sc_ctc_beam_job": _abi.BeamJob, "sc_beam_t": _abi.Beam,
               "sc_beam_lm_t": _abi.BeamLm}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "scasr.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)],
                   check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(out[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(out[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    # the sizes the backend's numpy views and the compiler are written against; the old structs keep theirs, the plain
    # job leads the new one
    assert (int(out["sc_beam_gr_t"]), int(out["sc_grammar_header"]), int(out["sc_ctc_beam_gr_job"])) == (64, 32, 96)
    assert (int(out["sc_ctc_beam_job"]), int(out["sc_beam_t"]), int(out["sc_beam_lm_t"])) == (72, 528, 192)
    assert int(out["sc_ctc_beam_gr_job.beam"]) == 0 and 4 * grammar.HEADER_WORDS == 32
    blob = grammar.compile([[1, 2], [1]], 4, 0)                      # start -1-> A(accept) -2-> B(accept); A, B loop to 1
    head = _abi.GrammarHeader.from_buffer_copy(blob[:32])
    assert (head.magic, head.version, head.V, head.blank, head.n_states, head.n_arcs, head.start_state, head.reserved) == \
        (_abi.GRAMMAR_MAGIC, _abi.GRAMMAR_VERSION, 4, 0, 3, 4, 0, 0)
    assert blob[:4] == b"SCGR" and len(blob) == 32 + 16 + 16 + 16 + 16
    assert struct.unpack_from("<4i", blob, 32) == (0, 1, 3, 4)                       # arc_off
    assert struct.unpack_from("<4i", blob, 48) == (1, 1, 2, 1)                       # arc_tok
    assert struct.unpack_from("<4i", blob, 64) == (1, 1, 2, 1)                       # arc_next
    assert struct.unpack_from("<3i", blob, 80) == (0, 1, 1)                          # accept


def test_constants_match_the_header_and_the_abi_revision_stays():
    from speechcatcher_amd import _abi, grammar
    hdr = (ROOT / "include" / "scasr.h").read_text()
    define = lambda name: re.search(rf"#define {name} (.+?)(?: /\*|$)", hdr, re.M).group(1).strip()   # noqa: E731
    assert int(define("SC_GRAMMAR_MAGIC"), 0) == _abi.GRAMMAR_MAGIC == grammar.MAGIC
    assert int(define("SC_GRAMMAR_VERSION")) == _abi.GRAMMAR_VERSION == grammar.VERSION
    assert eval(define("SC_GRAMMAR_MAX_STATES")) == _abi.GRAMMAR_MAX_STATES == grammar.MAX_STATES == 1 << 20
    assert eval(define("SC_GRAMMAR_MAX_ARCS")) == _abi.GRAMMAR_MAX_ARCS == grammar.MAX_ARCS == 1 << 24
    assert int(define("SC_ABI_VERSION")) == _abi.ABI_VERSION == 12   # new symbols only: no struct of revision 12 changed
    for name in ("sc_ctc_beam_grammar", "sc_grammar_create", "sc_grammar_destroy", "sc_grammar_device_view"):
        assert name in _abi.EXPORTED_SYMBOLS and re.search(rf"\b{name}\(", hdr), name


def test_argument_errors_return_before_any_launch_or_allocation():
    from speechcatcher_amd import _abi, grammar
    if not _abi.LIB_PATH.exists():
        _abi.build()
    lib = _abi.load()
    fn = lib.sc_ctc_beam_grammar
    assert fn(None, 0, None) == 0
    assert fn(None, 2, None) == -1 and b"null job table" in lib.sc_last_error()
    assert fn(None, -1, None) == -1 and b"negative" in lib.sc_last_error()
    assert fn(ctypes.c_void_p(64), _abi.BEAM_MAX_JOBS + 1, None) == -1 and b"SC_BEAM_MAX_JOBS" in lib.sc_last_error()
    good = grammar.compile([[1, 2], [1]], 4, 0)
    handle = ctypes.c_void_p(77)
    for bad, why in ((good[:-1], b"size"), (b"", b"header"), (good[:8] + b"\xff" * 4 + good[12:], b"header"),
                     (good[:64] + struct.pack("<i", 3) + good[68:], b"next"),
                     (good[:48] + struct.pack("<i", 0) + good[52:], b"blank"),
                     (good[:52] + struct.pack("<ii", 2, 1) + good[60:], b"ascending"),
                     (good[:80] + struct.pack("<i", 2) + good[84:], b"accept")):
        buf = ctypes.create_string_buffer(bad, max(len(bad), 1))
        assert lib.sc_grammar_create(buf, len(bad), ctypes.byref(handle)) == -1, why
        assert why in lib.sc_last_error() and b"grammar blob" in lib.sc_last_error() and handle.value is None, why
    assert lib.sc_grammar_create(None, 10, ctypes.byref(handle)) == -1 and lib.sc_grammar_create(good, len(good), None) == -1
    assert lib.sc_grammar_destroy(None) == 0
    assert lib.sc_grammar_device_view(None, None, None) == -1 and b"null grammar" in lib.sc_last_error()
    assert lib.sc_grammar_use(None, 1) == -1 and lib.sc_grammar_step(None, 0, 1) == -1 and lib.sc_grammar_accepts(None, 0) == -1
