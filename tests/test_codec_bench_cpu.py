"""tools/codec_bench.py, the parsers the bench scripts share: the `run ...` lines of the host test programs' time_ commands by field name,
and dxtexconv's -timing line. The lines are the programs' printf formats with values filled in. No device, no child process."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import codec_bench as B  # noqa: E402

BOTH = "run 2 resident 1.250 ms up 111 down 22 host 3.500 ms up 3333 down 4"
SIDES = {"run": 2, "resident": 1.25, "resident up": 111, "resident down": 22, "host": 3.5, "host up": 3333, "host down": 4}


@pytest.mark.parametrize("line, want", [
    (BOTH, SIDES),                                                                                      # pnm_, png_ and jpeg_host_test time_load / time_save
    (BOTH + " file 98765", {**SIDES, "file": 98765}),                                                   # jpeg_write_host_test time_save
    (BOTH + " raw 0.750 ms undo 12.125 ms", {**SIDES, "raw": 0.75, "undo": 12.125}),                    # exr_host_test time_load / time_save
    (BOTH + " raw 0.750 ms undo 12.125 ms undo_gpu 0.0625 ms texels_gpu 0.1250 ms",
     {**SIDES, "raw": 0.75, "undo": 12.125, "undo_gpu": 0.0625, "texels_gpu": 0.125}),                  # tiff_host_test time_load
    ("run 0 raw 41.500 ms file 1000 rows 50331648", {"run": 0, "raw": 41.5, "file": 1000, "rows": 50331648}),                    # png_host_test time_raw
    ("run 4 raw 9.000 ms file 2000 coefficients 3000", {"run": 4, "raw": 9.0, "file": 2000, "coefficients": 3000}),              # jpeg_ and jpeg_write_host_test
])
def test_a_run_line_comes_back_by_field_name(line, want):
    assert B.parse_runs("not a run line\n" + line + "\n") == [want]


def test_the_bytes_belong_to_the_side_they_follow():
    row, = B.parse_runs("run 0 resident 1.000 ms up 1 down 2 host 2.000 ms up 3 down 4 raw 5.000 ms")
    assert (row["resident up"], row["resident down"], row["host up"], row["host down"]) == (1, 2, 3, 4)
    assert B.summary([row])["resident up/down"] == [1, 2] and B.summary([row])["host path up/down"] == [3, 4]


@pytest.mark.parametrize("line", [
    "run 0 resident 1.000 ms up 1 down 2",                                      # no host side
    "run 0 resident 1.000 ms up 1 host 2.000 ms up 3 down 4",                   # no down of the resident side
    "run 0 resident 1.000 ms up 1 down 2 host 2.000 ms up 3",                   # no down of the host side
    "run 0 resident 1.000 ms up 1 down 2 host 2.000 ms up 3 down",              # cut after a name
    "run 0 resident 1.000 up 1 down 2 host 2.000 ms up 3 down 4",               # no unit
    "run 0 resident 1.000 ms up 1 down 2 host 2.000 ms up 3 down 4 raw",        # cut after a name
    "run 0 resident 1.000 ms up 1 down 2 host 2.000 ms up 3 down 4 news 5",     # a field nobody knows
    "run 0",
])
def test_a_line_with_a_missing_field_raises(line):
    with pytest.raises(ValueError):
        B.parse_runs(line)


def test_the_timing_line_of_dxtexconv():
    out = "reading /tmp/in file.tga\n  /tmp/in file.tga: 12.375 ms, host -> device 50331666 bytes, device -> host 67108864 bytes\n"
    assert B.parse_timing(out) == (12.375, 50331666, 67108864)
    with pytest.raises(AssertionError):
        B.parse_timing("  /tmp/in.tga: 12.375 ms, host -> device 50331666 bytes\n")
