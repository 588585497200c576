"""The struct of consensus finals (include/scasr.h: sc_mbr_job) against its ctypes mirror in speechcatcher_amd/_abi.py:
the C compiler's size and field offsets, the constants, the unchanged ABI revision, the workspace size function, and the
argument errors that return before any launch (no GPU needed)."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_struct_layout_matches_ctypes(tmp_path):
    from speechcatcher_amd import _abi
    gcc = shutil.which("gcc")
    assert gcc is not None, "the C compiler is the yardstick of this test: gcc is needed"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "scasr.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(sc_mbr_job));']
    for fname, _ in _abi.MbrJob._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(sc_mbr_job, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(_abi.MbrJob) == 184
    for fname, _ in _abi.MbrJob._fields_:
        assert int(out[fname]) == getattr(_abi.MbrJob, fname).offset, fname


def test_constants_match_the_header_the_contract_and_the_abi_revision_stays():
    import mbr_ref as M
    from speechcatcher_amd import _abi, mbr
    hdr = (ROOT / "include" / "scasr.h").read_text()
    define = lambda name: int(re.search(rf"#define {name} \(?(-?(?:0x)?[0-9A-Fa-f]+)", hdr).group(1), 0)   # noqa: E731
    assert define("SC_MBR_MAX_HYPS") == _abi.MBR_MAX_HYPS == M.MAX_HYPS == mbr.MAX_HYPS == 16
    assert define("SC_MBR_MAX_LEN") == _abi.MBR_MAX_LEN == M.MAX_LEN >= 1024
    assert define("SC_MBR_MAX_JOBS") == _abi.MBR_MAX_JOBS
    assert (define("SC_MBR_NONFINITE"), define("SC_MBR_BAD_TOKEN"), define("SC_MBR_TOO_LONG"), define("SC_MBR_NO_PIVOT")) == \
        (_abi.MBR_NONFINITE, _abi.MBR_BAD_TOKEN, _abi.MBR_TOO_LONG, _abi.MBR_NO_PIVOT) == \
        (M.NONFINITE, M.BAD_TOKEN, M.TOO_LONG, M.NO_PIVOT)
    assert define("SC_ABI_VERSION") == _abi.ABI_VERSION == 12        # new symbols and structs only


def _lib():
    from speechcatcher_amd import _abi
    if not _abi.LIB_PATH.exists():
        _abi.build()
    return _abi.load()


def test_workspace_size():
    from speechcatcher_amd import _abi
    fn = _lib().sc_mbr_ws_bytes
    assert fn(0, 100) == 0 and fn(-1, 100) == 0 and fn(1, -1) == 0 and fn(_abi.MBR_MAX_JOBS + 1, 1) == 0
    one = fn(1, 400)
    assert fn(7, 400) == 7 * one and one % 256 == 0
    # 2 bits a cell, 4 cells a byte, 64 lanes of ceil(ceil(401 / 64) / 4) = 2 bytes per table row, 16 rows of 400 table rows
    assert 16 * 400 * 2 * 64 <= one <= 16 * 400 * 2 * 64 + 16 * 400 * 4 + 16 * 401 + 18 * 256
    assert fn(1, _abi.MBR_MAX_LEN) == fn(1, _abi.MBR_MAX_LEN + 500) <= 8 << 20      # what SC_MBR_WS_MIN_BYTES promises
    assert fn(1, 0) > 0


def test_argument_errors_return_before_any_launch():
    from speechcatcher_amd import _abi
    lib = _lib()
    fn = lib.sc_mbr
    assert fn(None, 0, None, 0, None) == 0
    assert fn(None, 2, None, 0, None) == -1 and b"null job table" in lib.sc_last_error()
    assert fn(None, -1, None, 0, None) == -1 and b"negative" in lib.sc_last_error()
    assert fn(ctypes.c_void_p(64), 1, None, 0, None) == -1 and b"null workspace" in lib.sc_last_error()
    assert fn(ctypes.c_void_p(64), _abi.MBR_MAX_JOBS + 1, ctypes.c_void_p(64), 0, None) == -1
    assert b"SC_MBR_MAX_JOBS" in lib.sc_last_error()
    nh = (ctypes.c_int * 1)()
    none10 = [None] * 10
    assert lib.sc_mbr_hyps(None, None, 0, 1, 1.0, 0, 1, *none10, nh) == -1
    assert lib.sc_mbr_lists(None, None, None, None, 0, None, None, 0, 1, 1, 1.0, *none10) == -1
    assert lib.sc_streams_set_mbr_ws(None, 1 << 30) == -1 and lib.sc_streams_mbr_ws(None, None, None) == -1
