"""bench.py's options without a GPU: a plain run is the headline alone, everything that takes runs of its own is behind
--full."""
import pytest

import bench


def test_a_plain_run_is_the_headline_alone():
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not a.full and a.legs == "none" and a.roofline_steps == 2 and a.roofline_csv == ""
    assert bench.parse_args(["--legs", "none"]).legs == "none"


def test_full_runs_the_legs():
    assert bench.parse_args(["--full"]).legs == "core"
    assert bench.parse_args(["--full", "--legs", "all"]).legs == "all"
    assert bench.parse_args(["--full", "--legs", "none", "--roofline-csv", "x.csv"]).roofline_csv == "x.csv"


@pytest.mark.parametrize("argv", [["--legs", "core"], ["--legs", "all"], ["--roofline-csv", "x.csv"]])
def test_what_moved_behind_full_is_refused_without_it(argv, capsys):
    with pytest.raises(SystemExit) as e:
        bench.parse_args(argv)
    assert e.value.code == 2 and "--full" in capsys.readouterr().err
