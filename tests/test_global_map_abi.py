"""The global-map additions to the C-ABI, without a GPU: symbols, structure sizes against the
header, defaults, and the PointXYZIRPYT ASCII writer (transformations.pcd)."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import REPO
from feature_base_pointcloud_registration_amd import api, build
from feature_base_pointcloud_registration_amd.fbr_types import KEYPOSE, FbrGmapParams, FbrGmapResult, gmap_params

NEW = ["fbr_gmap_params_default", "fbr_global_map_build", "fbr_global_map_get", "fbr_global_map_install",
       "fbr_global_map_save", "fbr_pcd_write_poses_ascii", "fbr_selftest_voxel_wide"]


def test_symbols_are_declared_exported_and_listed():
    lib = ctypes.CDLL(api.lib_path())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "fbr.h")).read(), flags=re.S)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in api.EXPORTED_SYMBOLS, s
        assert re.search(r"\b%s\s*\(" % s, src), s
    assert api.lib().fbr_abi_version() == 4  # additions only


def test_structure_sizes_equal_the_headers(tmp_path):
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fbr.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(fbr_gmap_params), sizeof(fbr_gmap_result),\n'
                   '  offsetof(fbr_gmap_params, wide), offsetof(fbr_gmap_result, n_dropped), offsetof(fbr_gmap_result, corner_wide));\n'
                   '  return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["g++", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(FbrGmapParams), ctypes.sizeof(FbrGmapResult), FbrGmapParams.wide.offset,
                   FbrGmapResult.n_dropped.offset, FbrGmapResult.corner_wide.offset]
    assert got[:2] == [32, 64]


def test_defaults_are_as_documented():
    p = FbrGmapParams(1.0, 2.0, 3, 4, (5, 6, 7, 8))
    api.lib().fbr_gmap_params_default(ctypes.byref(p))
    q = gmap_params()
    for name, _ in FbrGmapParams._fields_:
        a, b = getattr(p, name), getattr(q, name)
        assert (list(a) == list(b)) if name == "reserved_" else (a == b), name
    assert (p.corner_leaf, p.surf_leaf, p.wide, p.keep_raw, list(p.reserved_)) == (0.0, 0.0, 0, 0, [0, 0, 0, 0])


def parse_pcd_ascii(path):
    """Header as {KEY: [tokens]} and the data rows as lists of tokens."""
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    lines = lines[:-1]
    k = next(i for i, ln in enumerate(lines) if ln.startswith("DATA"))
    header = {}
    for ln in lines[:k + 1]:
        if ln.startswith("#"):
            continue
        t = ln.split(" ")
        header[t[0]] = t[1:]
    return header, [ln.split(" ") for ln in lines[k + 1:]]


def test_pcd_write_poses_header_and_rows(tmp_path):
    poses = np.zeros(3, KEYPOSE)
    poses[0] = (1.5, -2.25, 0.125, 0.0, 0.01, -0.02, 3.0, 0.0, 12.5)
    poses[1] = (123456.789, np.nan, -0.000123456789, 1.0, 1.0 / 3.0, 0.0, -3.1415927, 0.0, 1700000000.123456)
    poses[2] = (0.0, 1e-9, 1e10, 2.0, 0.5, 0.25, 0.125, 0.0, 1234567890.0)
    path = tmp_path / "transformations.pcd"
    api.pcd_write_poses(str(path), poses)
    header, rows = parse_pcd_ascii(path)
    assert header == {"VERSION": ["0.7"], "FIELDS": "x y z intensity roll pitch yaw time".split(),
                      "SIZE": "4 4 4 4 4 4 4 8".split(), "TYPE": ["F"] * 8, "COUNT": ["1"] * 8, "WIDTH": ["3"],
                      "HEIGHT": ["1"], "VIEWPOINT": "0 0 0 1 0 0 0".split(), "POINTS": ["3"], "DATA": ["ascii"]}
    assert open(path).readline() == "# .PCD v0.7 - Point Cloud Data file format\n"
    assert len(rows) == 3
    names = ["x", "y", "z", "intensity", "roll", "pitch", "yaw", "time"]
    for row, p in zip(rows, poses):
        want = ["nan" if np.isnan(p[n]) else "%.8g" % float(p[n]) for n in names]  # 8 significant digits, nan spelled out
        assert row == want
    assert rows[1][1] == "nan" and rows[1][7] == "1.7e+09" and rows[2][7] == "1.2345679e+09"
    assert rows[0] == ["1.5", "-2.25", "0.125", "0", "0.0099999998", "-0.02", "3", "12.5"]
    # the x, y, z, intensity columns are what the PointXYZI reader takes from such a file
    back = api.pcd_read(str(path))
    assert np.array_equal(back["x"][[0, 2]], poses["x"][[0, 2]]) and np.isnan(back["y"][1])
    assert np.array_equal(back["intensity"], poses["intensity"])


def test_pcd_write_poses_empty_and_bad_path(tmp_path):
    api.pcd_write_poses(str(tmp_path / "e.pcd"), np.zeros(0, KEYPOSE))
    header, rows = parse_pcd_ascii(tmp_path / "e.pcd")
    assert header["POINTS"] == ["0"] and rows == []
    try:
        api.pcd_write_poses(str(tmp_path / "missing" / "e.pcd"), np.zeros(1, KEYPOSE))
        raise AssertionError("no error")
    except api.FbrError as e:
        assert e.status == -1


def test_build_lists_the_new_sources():
    assert "fbr_gmap.hip" in build.HIP_SOURCES and "k_gmap.hip" in build.HIP_SOURCES
