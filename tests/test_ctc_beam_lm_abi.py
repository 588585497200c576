"""The structs of the language model fusion (include/scasr.h: sc_beam_lm_t, sc_ctc_beam_lm_job, sc_lm_header, sc_lm_slot,
sc_lm_view) against their ctypes mirrors in speechcatcher_amd/_abi.py and against the blob speechcatcher_amd/ngram.py
packs: the C compiler's sizes and field offsets, the constants, and the argument errors that return before any launch
or allocation (no GPU needed)."""
import ctypes
import re
import shutil
import struct
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_struct_layouts_match_ctypes_and_the_packer(tmp_path):
    from speechcatcher_amd import _abi, ngram
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    structs = {"sc_beam_lm_t": _abi.BeamLm, "sc_ctc_beam_lm_job": _abi.BeamLmJob, "sc_lm_header": _abi.LmHeader,
               "sc_lm_slot": _abi.LmSlot, "sc_lm_view": _abi.LmView, "sc_ctc_beam_job": _abi.BeamJob, "sc_beam_t": _abi.Beam}
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
    # the sizes the backend's numpy views and the packer are written against; the plain job keeps its layout, and leads
    assert (int(out["sc_beam_lm_t"]), int(out["sc_lm_slot"]), int(out["sc_lm_header"])) == (192, 24, 32)
    assert (int(out["sc_ctc_beam_job"]), int(out["sc_beam_t"]), int(out["sc_ctc_beam_lm_job.beam"])) == (72, 528, 0)
    assert (ngram.SLOT_BYTES, ngram.SLOT_DT.itemsize, 4 * ngram.HEADER_WORDS) == (24, 24, 32)
    assert [ngram.SLOT_DT.fields[n][1] for n in ("key", "logp", "next")] == [0, 8, 16]
    blob = ngram.pack({(1,): (-1.0, -0.5), (1, 2): (-0.25, 0.0)}, 4, bos=1)
    head = _abi.LmHeader.from_buffer_copy(blob[:32])
    assert (head.magic, head.version, head.V, head.order, head.n_states, head.n_arcs, head.n_slots, head.start_state) == \
        (_abi.LM_MAGIC, _abi.LM_VERSION, 4, 2, 2, 1, 2, 1)
    assert len(blob) == 32 + 8 * 2 + 8 + 8 * 4 + 16 + 24 * 2
    used = [s for s in (_abi.LmSlot.from_buffer_copy(blob[-48:-24]), _abi.LmSlot.from_buffer_copy(blob[-24:]))
            if s.key != ngram.EMPTY]
    assert [(s.key, s.logp, s.next, s.reserved) for s in used] == [((1 << 32) | 2, -0.25, 0, 0)]
    assert struct.unpack_from("<d", blob, 32 + 8)[0] == -0.5         # backoff of state 1


def test_constants_match_the_header_and_the_abi_revision_stays():
    from speechcatcher_amd import _abi, ngram
    hdr = (ROOT / "include" / "scasr.h").read_text()
    define = lambda name: int(re.search(rf"#define {name} \(?(-?(?:0x)?[0-9A-Fa-f]+)", hdr).group(1), 0)   # noqa: E731
    assert define("SC_LM_MAX_ORDER") == _abi.LM_MAX_ORDER == ngram.MAX_ORDER == 5
    assert define("SC_LM_MAGIC") == _abi.LM_MAGIC == ngram.MAGIC
    assert define("SC_LM_VERSION") == _abi.LM_VERSION == ngram.VERSION
    assert define("SC_LM_EMPTY") == ngram.EMPTY and define("SC_LM_HASH_MUL") == ngram.HASH_MUL
    assert define("SC_ABI_VERSION") == _abi.ABI_VERSION == 12        # new symbols only: no struct of revision 12 changed


def test_argument_errors_return_before_any_launch_or_allocation():
    from speechcatcher_amd import _abi, ngram
    if not _abi.LIB_PATH.exists():
        _abi.build()
    lib = _abi.load()
    fn = lib.sc_ctc_beam_lm
    assert fn(None, 0, None) == 0
    assert fn(None, 2, None) == -1 and b"null job table" in lib.sc_last_error()
    assert fn(None, -1, None) == -1 and b"negative" in lib.sc_last_error()
    assert fn(ctypes.c_void_p(64), _abi.BEAM_MAX_JOBS + 1, None) == -1 and b"SC_BEAM_MAX_JOBS" in lib.sc_last_error()
    good = ngram.pack({(1,): (-1.0, -0.5), (1, 2): (-0.25, 0.0)}, 4)
    handle = ctypes.c_void_p(77)
    for bad, why in ((good[:-1], b"size"), (b"", b"header"), (good[:8] + b"\xff" * 4 + good[12:], b"header"),
                     (good[:-32] + struct.pack("<ii", 5, 0) + good[-24:-8] + struct.pack("<ii", 5, 0), b"next")):
        buf = ctypes.create_string_buffer(bad, max(len(bad), 1))
        assert lib.sc_lm_create(buf, len(bad), ctypes.byref(handle)) == -1, why
        assert why in lib.sc_last_error() and b"language model blob" in lib.sc_last_error() and handle.value is None
    assert lib.sc_lm_create(None, 10, ctypes.byref(handle)) == -1 and lib.sc_lm_create(good, len(good), None) == -1
    lib.sc_lm_destroy(None)
    assert lib.sc_lm_device_view(None, None, None) == -1 and b"null model" in lib.sc_last_error()
