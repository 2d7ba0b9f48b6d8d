"""Malaria-infected cells and STL meshes without a GPU: the reference's malaria drivers and cell_shapes compile unchanged
against the facade, the repository's malaria driver links against libhemocell_amd.so, the C ABI names the new model,
construct type and entry points, and the fixtures are the reference's data."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("HEMOCELL_REFERENCE", "/root/reference")
CASE = os.path.join(ROOT, "tests", "golden", "malaria_case")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hemocell_amd", "compat")]
DRIVERS = ["cases/stretchMalaria/stretchMalaria.cpp", "cases/pipeflowMalaria/pipeflowMalaria.cpp",
           "examples/cell_shapes/cell_shapes.cpp"]


@pytest.mark.parametrize("driver", DRIVERS)
def test_reference_malaria_driver_compiles_unchanged(driver):
    src = os.path.join(REF, driver)
    if not os.path.exists(src):
        pytest.skip("reference tree not present (it does not travel to the GPU box)")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-DHEMOCELL_COMPAT_MAIN", "-Wno-deprecated-declarations"] + INC + [src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_malaria_example_driver_links(tmp_path):
    from hemocell_amd import capi
    out = str(tmp_path / "stretch_malaria")
    libdir = os.path.dirname(capi.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wno-deprecated-declarations"] + INC +
                       [os.path.join(ROOT, "examples", "malaria", "stretch_malaria.cpp"), "-o", out, "-L" + libdir, "-lhemocell_amd",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_header_defines_the_malaria_model_and_stl_construct_type():
    src = open(os.path.join(ROOT, "include", "hemocell_amd.h")).read()
    defs = dict(re.findall(r"^#define (HC_\w+) (\d+)", src, flags=re.M))
    assert defs["HC_SHAPE_MESH_FROM_STL"] == "2"   # config/constant_defaults.h:84
    assert defs["HC_MODEL_RBC_MALARIA"] == "3"
    for sym in ("hcp_celltype_create_ex", "hcp_celltype_malaria_constants", "hc_celltype_spec"):
        assert sym in src
    from hemocell_amd import capi, host
    assert (host.MODEL_RBC_MALARIA, host.MESH_FROM_STL) == (3, 2)
    names = [f[0] for f in capi.CellTypeSpec._fields_]
    assert names == ["model", "shape", "material", "wbc", "kInnerLink", "stl_path"]


def test_malaria_fixture_material():
    """CellType.malaria's defaults: cases/stretchMalaria/RBC_MALARIA.xml (identical in pipeflowMalaria)"""
    from hemocell_amd import host
    m = host.read_material(host.MALARIA_XML)
    assert m["kInnerLink"] == 15.0 and m["kVolume"] == -0.5 and m["eta_m"] == 0.0 and m["radius"] == 5.4e-6
    assert m["kLink"] == 15.0 and m["kArea"] == 3.0 and m["kBend"] == 60.0
    ie = m["inner_edges"]
    assert ie.shape == (525, 2) and ie.min() >= 0 and ie.max() == 1502
    assert np.bincount(ie.reshape(-1)).max() <= 2
    assert host.read_stl_file_tag(host.MALARIA_XML) == "vRBC_uniform.stl"


@pytest.mark.parametrize("name,ntri", [("vRBC_uniform.stl", 3010), ("vRBC_uniform_pipeflowMalaria.stl", 3014)])
def test_stl_fixtures_are_binary_closed_meshes(name, ntri):
    raw = open(os.path.join(CASE, name), "rb").read()
    assert not raw.startswith(b"solid")
    n = int(np.frombuffer(raw[80:84], np.uint32)[0])
    assert n == ntri and len(raw) == 84 + 50 * n
