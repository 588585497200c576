"""The struct of n-gram rescoring (include/scasr.h: sc_lm_rescore_job) against its ctypes mirror in
speechcatcher_amd/_abi.py: the C compiler's size and field offsets, the constants, the unchanged ABI revision, and the
argument errors that return before any launch (no GPU needed)."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_struct_layout_matches_ctypes(tmp_path):
    from speechcatcher_amd import _abi
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "scasr.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(sc_lm_rescore_job));']
    for fname, _ in _abi.RescoreJob._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(sc_lm_rescore_job, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(_abi.RescoreJob) == 160
    for fname, _ in _abi.RescoreJob._fields_:
        assert int(out[fname]) == getattr(_abi.RescoreJob, fname).offset, fname


def test_constants_match_the_header_the_contract_and_the_abi_revision_stays():
    import lm_rescore_ref as RS
    from speechcatcher_amd import _abi, rescore
    hdr = (ROOT / "include" / "scasr.h").read_text()
    define = lambda name: int(re.search(rf"#define {name} \(?(-?(?:0x)?[0-9A-Fa-f]+)", hdr).group(1), 0)   # noqa: E731
    assert define("SC_RESCORE_MAX_HYPS") == _abi.RESCORE_MAX_HYPS == RS.MAX_HYPS == rescore.MAX_HYPS == 16
    assert define("SC_RESCORE_MAX_JOBS") == _abi.RESCORE_MAX_JOBS
    assert define("SC_RESCORE_FORCE_SERIAL") == _abi.RESCORE_FORCE_SERIAL == RS.FORCE_SERIAL
    assert (define("SC_RESCORE_NONFINITE"), define("SC_RESCORE_BAD_TOKEN"), define("SC_RESCORE_SERIAL")) == \
        (_abi.RESCORE_NONFINITE, _abi.RESCORE_BAD_TOKEN, _abi.RESCORE_SERIAL) == (RS.NONFINITE, RS.BAD_TOKEN, RS.SERIAL)
    assert define("SC_ABI_VERSION") == _abi.ABI_VERSION == 12        # new symbols only: no struct of revision 12 changed


def test_argument_errors_return_before_any_launch():
    from speechcatcher_amd import _abi
    if not _abi.LIB_PATH.exists():
        _abi.build()
    lib = _abi.load()
    fn = lib.sc_lm_rescore
    assert fn(None, 0, None) == 0
    assert fn(None, 2, None) == -1 and b"null job table" in lib.sc_last_error()
    assert fn(None, -1, None) == -1 and b"negative" in lib.sc_last_error()
    assert fn(ctypes.c_void_p(64), _abi.RESCORE_MAX_JOBS + 1, None) == -1 and b"SC_RESCORE_MAX_JOBS" in lib.sc_last_error()
    nh = (ctypes.c_int * 1)()
    assert lib.sc_rescore_hyps(None, None, 0, 1, None, 0.5, 0.0, -1, None, None, None, None, None, None, nh) == -1
    assert lib.sc_lm_rescore_lists(None, None, None, None, None, None, 0, 1, 1, None, 0.5, 0.0, -1, None, None, None, None,
                                   None, None) == -1
