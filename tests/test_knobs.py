"""The environment knobs (csrc/fbr_knobs.h): what each parse gives for values below, inside and
above its range, and that the header and the table in DESIGN.md §6 "Tuning knobs" list the same
knobs in the same order with the same defaults.

Most knobs are read once per process, so every environment gets a child Python process, which
loads the host probe library (tests/native/host_probe.cpp, probe_knobs) and prints the values.

The expectations below were written from the getenv blocks the knobs had before they moved into
the header (one block per knob, spread over fbr_api.hip, fbr_gn.h and five k_*.hip files), not from
the header: they pin those mappings.
"""
import json
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "feature_base_pointcloud_registration_amd", "csrc", "fbr_knobs.h")
DESIGN = os.path.join(REPO, "DESIGN.md")

# (knob, [(value, result), ...]) for the three set environments: an in-range non-default value; a
# value below the range (or zero where zero is special); a value above it or text.  Flags are "any
# value atoi reads as non-zero": -1 and 7 are on, text is off.  The cell sizes are in metres and
# come back as 8 / (the power of two they round to, clamped); a cell of 0 or text is ignored.
CASES = [
    ("FBR_NSUB", [("2", 2), ("0", 1), ("99", 8)]),                       # max(1, min(8, .)); unset 0
    ("FBR_KNN_TILE", [("1", 1), ("0", 0), ("abc", 0)]),
    ("FBR_KNN_TILE_STATS", [("1", 1), ("0", 0), ("abc", 0)]),
    ("FBR_VG_SPLIT", [("4", 4), ("0", 1), ("64", 8)]),                    # below 2 gives 1, else min(p, 8)
    ("FBR_INGEST_COMPACT", [("0", 0), ("-1", 1), ("abc", 0)]),
    ("FBR_COPY_SPIN_US", [("250", 250), ("-5", 0), ("abc", 0)]),          # max(0, .)
    ("FBR_COMPACT_CELLS", [("1024", 1024), ("100", 512), ("4096", 2048)]),
    ("FBR_GN_GRID", [("4096", 4096), ("0", 1), ("abc", 1)]),              # max(1, .)
    ("FBR_GN_ONE_ITEM", [("0", 0), ("-1", 1), ("abc", 0)]),
    ("FBR_GN_TAIL_ONE_ITEM", [("0", 0), ("-1", 1), ("2", 1)]),
    ("FBR_GN_ONE_GRID", [("1000", 1000), ("-7", 1), ("1000000", 1000000)]),
    ("FBR_PACKED_SCANS", [("0", 0), ("-1", 1), ("7", 1)]),
    ("FBR_FEAT_COMPACT", [("0", 0), ("-1", 1), ("abc", 0)]),
    ("FBR_FEAT_SURF_WIN", [("64", 64), ("0", 64), ("abc", 64)]),          # 59 gives 59, anything else 64
    ("FBR_FEAT_SURF_WINDOW", [("0", 0), ("-1", 1), ("abc", 0)]),
    ("FBR_OWNER_TAGS", [("0", 0), ("-1", 1), ("yes", 0)]),
    ("FBR_OWNER_TMAX", [("3", 3), ("0", 0), ("abc", 0)]),                 # only a positive value caps
    ("FBR_GN_TAIL", [("4", 4), ("-2", 0), ("1000", 1000)]),               # max(0, .)
    ("FBR_GN_LAG", [("3", 3), ("0", 1), ("99", 8)]),                      # clamped to 1..8
    ("FBR_KNN_FLAT", [("0", 0), ("-1", 1), ("abc", 0)]),
    ("FBR_KNN_CELL", [("0.5", 16), ("0", 8), ("100", 4)]),                # 0.25 m .. 2 m
    ("FBR_KNN_CELL_X", [("0.5", 16), ("0.01", 64), ("abc", 32)]),         # 0.125 m .. 2 m
    ("FBR_VG_LARGE_MIN", [("1000", 1000), ("0", 1), ("abc", 1)]),         # max(1, .)
    ("FBR_VR_DBG", [("2", 2), ("-1", -1), ("abc", 0)]),                   # as atoi reads it
    ("FBR_VG_INPLACE", [("0", 0), ("-1", 1), ("abc", 0)]),
    ("FBR_VG_CLASSES", [("2", 2), ("-1", 1), ("3", 1)]),                  # outside 0..2 gives 1
    ("FBR_FIT_CACHE", [("0", 0), ("-1", -1), ("5", 5)]),                  # as atoi reads it
    ("FBR_GRID_SPARSE", [("1", 1), ("-1", 1), ("abc", 0)]),
    ("FBR_KNN_LPQ", [("8", 8), ("0", 1), ("100", 8)]),                    # >= 8 gives 8, any other set value 1
    ("FBR_FEAT_WAVES", [("3", 2), ("1", 1), ("9", 4)]),                   # >= 4: 4; 2, 3: 2; 1: 1; else unforced
    ("FBR_DIRECT", [("0", 0), ("-1", 1), ("abc", 0)]),
    ("FBR_PINNED_UPLOAD", [("0", 0), ("-1", 1), ("abc", 0)]),
    ("FBR_STAGE_MB", [("8", 8), ("0", 1), ("abc", 1)]),                   # max(1, .)
    ("FBR_STAGE_THREADS", [("4", 4), ("0", 1), ("1000", 1000)]),          # max(1, .); unset 0
    ("FBR_INGEST_XSTREAM", [("0", 0), ("-1", 1), ("abc", 0)]),
    ("FBR_INGEST_NT", [("0", 0), ("-1", 1), ("abc", 0)]),
]
NAMES = [name for name, _ in CASES]
# Further single values of the quantised knobs, one child more: the rest of the mappings above.
MORE = {"FBR_COMPACT_CELLS": ("2048", 2048), "FBR_FEAT_SURF_WIN": ("59", 59), "FBR_FEAT_WAVES": ("0", 0),
        "FBR_KNN_LPQ": ("abc", 1), "FBR_VG_SPLIT": ("1", 1), "FBR_VG_CLASSES": ("0", 0), "FBR_GN_LAG": ("-3", 1),
        "FBR_KNN_CELL": ("abc", 8), "FBR_KNN_CELL_X": ("100", 4)}

CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.probe_knobs.restype = ctypes.c_int64
out = (ctypes.c_int64 * 64)()
n = lib.probe_knobs(out)
print(json.dumps(list(out[:n])))
"""


def run_child(lib_path, env_set):
    env = {k: v for k, v in os.environ.items() if not k.startswith("FBR_")}
    env.update(env_set)
    r = subprocess.run([sys.executable, "-c", CHILD, lib_path], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def lib_path(probe_lib):
    return probe_lib._name


def header_knobs():
    with open(HEADER) as f:
        names = re.findall(r'"(FBR_[A-Z0-9_]+)"', f.read())
    assert len(names) == len(set(names)), "a knob is read in two places of fbr_knobs.h"
    return names


def design_rows():
    """[(knob, default as probe_knobs reports it)] of the table under "### Tuning knobs"."""
    with open(DESIGN) as f:
        text = f.read()
    sec = text[text.index("### Tuning knobs"):]
    sec = sec[:sec.index("\n## ")]
    rows = []
    for line in sec.split("\n"):
        m = re.match(r"\| `(FBR_[A-Z0-9_]+)` \| ([^|]+) \|", line)
        if not m:
            continue
        cell = m.group(2).strip()
        metres = re.match(r"([0-9.]+) m\b", cell)
        if cell.startswith("unset"):
            val = 0                              # "0 = not forced"
        elif metres:
            val = round(8 / float(metres.group(1)))
        else:
            val = int(re.match(r"-?\d+", cell).group(0))
        rows.append((m.group(1), val))
    return rows


def test_header_table_and_cases_list_the_same_knobs():
    hdr = header_knobs()
    assert [name for name, _ in design_rows()] == hdr   # a knob without a row, a row without a knob, the order
    assert NAMES == hdr


def test_defaults_match_the_design_table(lib_path):
    got = run_child(lib_path, {})
    rows = design_rows()
    assert len(got) == len(rows) + 2
    assert dict(zip(NAMES, got)) == dict(rows)
    assert got[len(rows):] == [16, 64]   # mapping leaves below 0.3 m: 0.5 m and 0.125 m cells


@pytest.mark.parametrize("which", [0, 1, 2], ids=["in_range", "below_or_zero", "above_or_text"])
def test_set_values_parse_as_before(lib_path, which):
    got = run_child(lib_path, {name: vals[which][0] for name, vals in CASES})
    want = {name: vals[which][1] for name, vals in CASES}
    assert dict(zip(NAMES, got)) == want
    # for mapping leaves below 0.3 m: a set cell size holds as well, an ignored one leaves 0.5 m / 0.125 m
    cells = {0: [16, 16], 1: [16, 64], 2: [4, 64]}[which]
    assert got[len(NAMES):] == cells


def test_further_values_of_the_quantised_knobs(lib_path):
    got = dict(zip(NAMES, run_child(lib_path, {name: v for name, (v, _) in MORE.items()})))
    assert {name: got[name] for name in MORE} == {name: want for name, (_, want) in MORE.items()}
