"""The structs of the CTC prefix beam search (include/scasr.h: sc_beam_entry, sc_beam_t, sc_beam_node, sc_ctc_beam_job,
sc_ctc_beam_pack_job) against their ctypes mirrors in speechcatcher_amd/_abi.py: the C compiler's sizes and field
offsets, the limits, and the argument errors that return before any launch (no GPU needed)."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_struct_layouts_match_ctypes(tmp_path):
    from speechcatcher_amd import _abi
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    structs = {"sc_beam_entry": _abi.BeamEntry, "sc_beam_t": _abi.Beam, "sc_beam_node": _abi.BeamNode,
               "sc_ctc_beam_job": _abi.BeamJob, "sc_ctc_beam_pack_job": _abi.BeamPackJob}
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
    # the sizes the backend's numpy views are written against
    assert (int(out["sc_beam_entry"]), int(out["sc_beam_t"]), int(out["sc_beam_node"])) == (32, 528, 16)


def test_limits_match_the_header():
    from speechcatcher_amd import _abi
    hdr = (ROOT / "include" / "scasr.h").read_text()
    define = lambda name: int(re.search(rf"#define {name} \(?(-?\d+)\)?", hdr).group(1))   # noqa: E731
    assert define("SC_BEAM_MAX") == _abi.BEAM_MAX == 16
    assert define("SC_BEAM_MAX_JOBS") == _abi.BEAM_MAX_JOBS
    assert [define(f"SC_BEAM_PACK_{n}") for n in ("OK", "NO_ENTRY", "TRUNCATED", "BROKEN")] == [
        _abi.BEAM_PACK_OK, _abi.BEAM_PACK_NO_ENTRY, _abi.BEAM_PACK_TRUNCATED, _abi.BEAM_PACK_BROKEN]


def test_argument_errors_return_before_any_launch():
    from speechcatcher_amd import _abi
    if not _abi.LIB_PATH.exists():
        _abi.build()
    lib = _abi.load()
    for fn in (lib.sc_ctc_beam, lib.sc_ctc_beam_pack):
        assert fn(None, 0, None) == 0
        assert fn(None, 2, None) == -1 and b"null job table" in lib.sc_last_error()
        assert fn(None, -1, None) == -1 and b"negative" in lib.sc_last_error()
        assert fn(ctypes.c_void_p(64), _abi.BEAM_MAX_JOBS + 1, None) == -1 and b"SC_BEAM_MAX_JOBS" in lib.sc_last_error()
