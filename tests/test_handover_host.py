"""The hand-over of the per-chunk side states (speechcatcher_amd/csrc/handover.h) without a GPU: tests/host/handover_check.cpp
- a stand-alone program that includes nothing but that header - drives the templates with a seeded schedule of admissions,
completions, reports and resets against a straight-line model, once with carriers that complete in order (encoder groups)
and once with carriers collected in any order (the input level's staging slots)."""
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_handover_templates_follow_the_model_under_a_scripted_schedule(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "handover_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(ROOT / "speechcatcher_amd" / "csrc"),
                    str(ROOT / "tests" / "host" / "handover_check.cpp"), "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.splitlines()[-1] == "handover ok", res.stdout
