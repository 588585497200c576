"""The structs of attention rescoring (include/scasr.h: sc_seq_attn_job, sc_dec_rescore_job) against their ctypes mirrors in
speechcatcher_amd/_abi.py: the C compiler's sizes and field offsets, the constants, the new symbols, the unchanged ABI
revision, and the argument errors that return before any launch (no GPU needed)."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
STRUCTS = (("sc_seq_attn_job", "SeqAttnJob", 80), ("sc_dec_rescore_job", "DecRescoreJob", 160))


@pytest.mark.parametrize("cname,pyname,size", STRUCTS)
def test_struct_layout_matches_ctypes(tmp_path, cname, pyname, size):
    from speechcatcher_amd import _abi
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    mirror = getattr(_abi, pyname)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "scasr.h"', "int main(void) {",
             f'  printf("size %zu\\n", sizeof({cname}));']
    for fname, _ in mirror._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(mirror) == size
    for fname, _ in mirror._fields_:
        assert int(out[fname]) == getattr(mirror, fname).offset, fname


def test_constants_match_the_header_the_contract_and_the_abi_revision_stays():
    import dec_rescore_ref as DR
    from speechcatcher_amd import _abi
    hdr = (ROOT / "include" / "scasr.h").read_text()
    define = lambda name: int(re.search(rf"#define {name} \(?(-?(?:0x)?[0-9A-Fa-f]+)", hdr).group(1), 0)   # noqa: E731
    assert define("SC_ATT_MAX_HYPS") == _abi.ATT_MAX_HYPS == DR.MAX_HYPS == 16
    assert define("SC_ATT_MAX_JOBS") == _abi.ATT_MAX_JOBS
    assert (define("SC_ATT_NONFINITE"), define("SC_ATT_BAD_TOKEN"), define("SC_ATT_TOO_LONG"), define("SC_ATT_NO_FRAMES")) == \
        (_abi.ATT_NONFINITE, _abi.ATT_BAD_TOKEN, _abi.ATT_TOO_LONG, _abi.ATT_NO_FRAMES) == \
        (DR.NONFINITE, DR.BAD_TOKEN, DR.TOO_LONG, DR.NO_FRAMES)
    assert define("SC_ERR_UNSUPPORTED") == _abi.ERR_UNSUPPORTED == -5 and define("SC_ERR_CAPACITY") == _abi.ERR_CAPACITY
    assert re.search(r"#define SC_SEQ_ATTN_MAX_JOBS \(1 << 24\)", hdr) and _abi.SEQ_ATTN_MAX_JOBS == 1 << 24
    assert define("SC_ABI_VERSION") == _abi.ABI_VERSION == 12        # new symbols only: no struct of revision 12 changed
    for name in ("sc_seq_attention", "sc_dec_rescore", "sc_dec_rescore_ws_bytes"):
        assert name in _abi.EXPORTED_SYMBOLS and re.search(rf"\b{name}\(", hdr), name


def _model(_abi, **over):
    """a model struct with plausible dims and every weight pointer set to a dummy address (nothing is launched)"""
    layers = (_abi.DecLayer * 2)()
    for i in range(2):
        for fname, _ in _abi.DecLayer._fields_:
            setattr(layers[i], fname, 256)
    s = _abi.Search()
    s.V, s.d, s.H, s.F, s.n_layers, s.LCAP, s.sos, s.eos, s.ln_eps = 1024, 64, 4, 2048, 2, 64, 1023, 1023, 1e-12
    for fname in ("embed", "pe", "dec_norm_g", "dec_norm_b", "out_w", "out_b"):
        setattr(s, fname, 256)
    s.layers = ctypes.cast(layers, ctypes.c_void_p).value
    for k, v in over.items():
        setattr(s, k, v)
    return s, layers


def test_argument_errors_return_before_any_launch():
    from speechcatcher_amd import _abi
    if not _abi.LIB_PATH.exists():
        _abi.build()
    lib = _abi.load()
    att = lib.sc_seq_attention
    assert att(None, 0, 16, 0, 1, 1, None) == 0
    assert att(None, 2, 16, 4, 1, 1, None) == -1 and b"null job table" in lib.sc_last_error()
    assert att(None, -1, 16, 4, 1, 1, None) == -1 and b"negative" in lib.sc_last_error()
    dummy = ctypes.c_void_p(256)
    assert att(dummy, 1, 24, 4, 1, 1, None) == -1 and b"head dim" in lib.sc_last_error()
    assert att(dummy, 1, 16, 4, 1, 0, None) == -1 and b"forms" in lib.sc_last_error()
    assert att(dummy, 1, 16, -1, 1, 1, None) == -1 and att(dummy, 1, 16, 4, 0, 1, None) == -1
    assert att(dummy, _abi.SEQ_ATTN_MAX_JOBS + 1, 16, 4, 1, 1, None) == -1 and b"SC_SEQ_ATTN_MAX_JOBS" in lib.sc_last_error()

    rs = lib.sc_dec_rescore
    s, keep = _model(_abi)
    sp = ctypes.addressof(s)
    assert rs(None, 0, sp, None, 0, None) == 0
    assert rs(None, 1, sp, dummy, 1 << 20, None) == -1 and b"null job table" in lib.sc_last_error()
    assert rs(None, -1, sp, dummy, 1 << 20, None) == -1 and b"negative" in lib.sc_last_error()
    assert rs(dummy, _abi.ATT_MAX_JOBS + 1, sp, dummy, 1 << 20, None) == -1 and b"SC_ATT_MAX_JOBS" in lib.sc_last_error()
    assert rs(dummy, 1, None, dummy, 1 << 20, None) == -1 and b"null model" in lib.sc_last_error()
    for over, text in (({"d": 48}, b"multiple of 32"), ({"H": 8}, b"head dim"), ({"V": 1 << 20}, b"bad model"), ({"sos": 1024}, b"sos")):
        bad, keep2 = _model(_abi, **over)
        assert rs(dummy, 1, ctypes.addressof(bad), dummy, 1 << 20, None) == -1 and text in lib.sc_last_error(), over
        assert lib.sc_dec_rescore_ws_bytes(ctypes.addressof(bad), 10, 10, 1, 1) == 0
    # a handle without the fp32 decoder weights: refused, whatever the jobs are
    keep[1].wq = None
    assert rs(dummy, 1, sp, dummy, 1 << 20, None) == _abi.ERR_UNSUPPORTED and b"fp32 decoder weights" in lib.sc_last_error()
    keep[1].wq = 256
    assert lib.sc_dec_rescore_ws_bytes(sp, 10, 10, 1, 1) > 10 * 1024 * 4

    # malformed jobs: SC_ERR_ARG, nothing is launched (the pointers are dummies)
    def job(**over):
        j = _abi.DecRescoreJob()
        for fname in ("E", "yseq", "score", "wkv", "bkv", "att", "fused", "order", "status"):
            setattr(j, fname, 256)
        j.e_stride, j.row_stride, j.score_stride, j.tok_stride = 64, 8, 1, 9
        j.w_att, j.w_ctc, j.beta = 1.0, 0.5, 0.0
        j.n_hyp, j.L, j.T, j.pe_rows = 2, 8, 5, 100
        for k, v in over.items():
            setattr(j, k, v)
        return j
    ws = ctypes.c_void_p(1 << 20)
    for over, text in (({"yseq": None}, b"null pointer"), ({"status": None}, b"null pointer"), ({"n_hyp": 0}, b"n_hyp"),
                       ({"n_hyp": 17}, b"n_hyp"), ({"L": -1}, b"out of range"), ({"T": -1}, b"out of range"),
                       ({"pe_rows": 0}, b"out of range"), ({"E": None}, b"encoder rows"), ({"E": 260}, b"encoder rows"),
                       ({"e_stride": 63}, b"encoder rows"), ({"row_stride": 7}, b"stride"), ({"score_stride": 0}, b"stride"),
                       ({"tok_att": 256, "tok_stride": 8}, b"stride"), ({"w_att": float("nan")}, b"not finite"),
                       ({"beta": float("inf")}, b"not finite")):
        tab = (_abi.DecRescoreJob * 1)(job(**over))
        assert rs(tab, 1, sp, ws, 1 << 30, None) == -1 and text in lib.sc_last_error(), over
    two = (_abi.DecRescoreJob * 2)(job(), job(wkv=512))
    assert rs(two, 2, sp, ws, 1 << 30, None) == -1 and b"differ" in lib.sc_last_error()
    one = (_abi.DecRescoreJob * 1)(job())
    assert rs(one, 1, sp, ctypes.c_void_p((1 << 20) + 8), 1 << 30, None) == -1 and b"aligned" in lib.sc_last_error()
    # a workspace that one job alone does not fit: SC_ERR_CAPACITY before any launch
    assert rs(one, 1, sp, ws, 4096, None) == _abi.ERR_CAPACITY and b"workspace" in lib.sc_last_error()
