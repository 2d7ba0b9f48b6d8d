"""White blood cells without a GPU: the reference's WBC drivers compile unchanged against the facade, the repository's
own WBC driver links against libhemocell_amd.so, and the C ABI names the new model and construct type."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("HEMOCELL_REFERENCE", "/root/reference")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hemocell_amd", "compat")]
WBC_DRIVERS = ["cases/cellCollision_sphere/cellCollision_sphere.cpp", "cases/flowchamber_stenosis/flowchamber_stenosis.cpp",
               "examples/cell_shapes/cell_shapes.cpp"]


@pytest.mark.parametrize("driver", WBC_DRIVERS)
def test_reference_wbc_driver_compiles_unchanged(driver):
    src = os.path.join(REF, driver)
    if not os.path.exists(src):
        pytest.skip("reference tree not present (it does not travel to the GPU box)")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-DHEMOCELL_COMPAT_MAIN", "-Wno-deprecated-declarations"] + INC + [src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_wbc_example_driver_links(tmp_path):
    from hemocell_amd import capi
    out = str(tmp_path / "wbc_collision")
    libdir = os.path.dirname(capi.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wno-deprecated-declarations"] + INC +
                       [os.path.join(ROOT, "examples", "wbc", "wbc_collision.cpp"), "-o", out, "-L" + libdir, "-lhemocell_amd",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_header_defines_the_wbc_model_and_construct_type():
    src = open(os.path.join(ROOT, "include", "hemocell_amd.h")).read()
    defs = dict(re.findall(r"^#define (HC_\w+) (\d+)", src, flags=re.M))
    assert defs["HC_SHAPE_WBC_SPHERE"] == "0"   # config/constant_defaults.h:83
    assert defs["HC_MODEL_WBC_HO"] not in (defs["HC_MODEL_RBC_HO"], defs["HC_MODEL_PLT_SIMPLE"])
    from hemocell_amd import host
    assert (host.MODEL_WBC_HO, host.WBC_SPHERE) == (int(defs["HC_MODEL_WBC_HO"]), 0)


def test_wbc_fixture_material():
    """CellType.wbc's defaults: the moduli, WBC constants and 321 inner edges of examples/cell_shapes/WBC_HO.xml"""
    from hemocell_amd import host
    m = host.read_material(host.WBC_HO_XML)
    assert m["kInnerRigid"] == 6.40625e-12 and m["kCytoskeleton"] == 6.40625e-15 and m["coreRadius"] == 2.5e-6 and m["radius"] == 4e-6
    assert m["inner_edges"].shape == (321, 2) and m["inner_edges"].min() == 0 and m["inner_edges"].max() == 641
    assert int(m["minNumTriangles"]) == 600 and m["eta_m"] == 1e-9
