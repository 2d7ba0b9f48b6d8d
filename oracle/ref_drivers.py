"""The drop-in check: the reference's OWN case drivers, compiled unchanged from where they lie in the reference tree
against this repository's facade (hemocell_amd/compat) and linked with libhemocell_amd.so.  TEST INFRASTRUCTURE ONLY.

Only possible where the reference tree is present (HEMOCELL_REFERENCE); elsewhere build() does nothing.  The binaries
land in oracle/_ref/ (git-ignored) and tests/test_gpu_compat_driver.py runs them.  Their library search paths are
relative to the binary ($ORIGIN) and the HDF5 libraries they use are copied next to them, so a tree copied to
another directory or machine still loads its own libhemocell_amd.so and needs no HDF5 installation."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "_ref")
REF = os.environ.get("HEMOCELL_REFERENCE", "/root/reference")
HDF5_INC, HDF5_LIB = "/opt/conda/include", "/opt/conda/lib"
DRIVERS = {"pipeflow": "examples/pipeflow/pipeflow.cpp", "stretchCell": "examples/stretchCell/stretchCell.cpp",
           "oneCellShear": "examples/oneCellShear/oneCellShear.cpp",
           "performance_testing": "cases/performance_testing/performance_testing.cpp",
           # more of the reference's drivers that stay inside the path (no pre-inlet, no interior viscosity, RBC / PLT models)
           "simple": "examples/simple/simple.cpp", "cube": "examples/cube/cube.cpp", "parachuting": "examples/parachuting/parachuting.cpp",
           "parallelplanes": "examples/parallelplanes/parallelplanes.cpp", "cellCollision": "cases/cellCollision/cellCollision.cpp",
           "kolmogorovFlow": "cases/kolmogorovFlow/kolmogorovFlow.cpp", "unbounded": "cases/unbounded/unbounded.cpp",
           # geometry from a plb::DomainFunctional3D the driver defines (sphere, stenosis, bent vessel, stent)
           "flowaroundsphere": "examples/flowaroundsphere/flowaroundsphere.cpp", "microcontraction": "examples/microcontraction/microcontraction.cpp",
           "stenosis": "cases/stenosis/stenosis.cpp", "stentflow": "cases/stentflow/stentflow.cpp",
           "microvessel_bended": "cases/microvessel_bended/microvessel_bended.cpp",
           "vasoconstriction_pipe": "cases/vasoconstriction_pipe/vasoconstriction_pipe.cpp", "atherosclerosis": "cases/atherosclerosis/atherosclerosis.cpp"}


def path(name):
    """where the binary of driver `name` is (it exists only after a build() that saw the reference tree)"""
    return os.path.join(OUT, name)


def build():
    if not os.path.isdir(REF):
        return
    os.makedirs(os.path.join(OUT, "hdf5lib"), exist_ok=True)
    libdir = os.path.join(ROOT, "hemocell_amd", "lib")
    hdf5 = []
    if os.path.exists(os.path.join(HDF5_INC, "hdf5.h")) and os.path.exists(os.path.join(HDF5_LIB, "libhdf5_hl.so.100")):
        # linked by path from a private directory: HDF5_LIB on the search path would also pull in conda's older
        # libstdc++.  The libraries are copied, not linked to, so the binaries run where HDF5_LIB does not exist
        # (the three need nothing else from it: their own search path is $ORIGIN)
        for lib in ("libhdf5.so.103", "libhdf5_hl.so.100", "libz.so.1"):
            dst = os.path.join(OUT, "hdf5lib", lib)
            if os.path.islink(dst):
                os.remove(dst)
            shutil.copyfile(os.path.join(HDF5_LIB, lib), dst)
        hdf5 = ["-DHEMOCELL_WITH_HDF5", "-I" + HDF5_INC, os.path.join(OUT, "hdf5lib", "libhdf5_hl.so.100"),
                os.path.join(OUT, "hdf5lib", "libhdf5.so.103"), "-Wl,-rpath,$ORIGIN/hdf5lib"]
    jobs = []
    for name, src in DRIVERS.items():
        base = ["g++", "-std=c++14", "-O2", "-Wno-deprecated-declarations", "-DHEMOCELL_COMPAT_MAIN",
                "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hemocell_amd", "compat"), os.path.join(REF, src)]
        link = ["-L" + libdir, "-lhemocell_amd", "-Wl,-rpath,$ORIGIN/" + os.path.relpath(libdir, OUT)]
        jobs.append(base + ["-o", path(name)] + link + hdf5)
        if name in ("pipeflow", "performance_testing", "unbounded") and hdf5:
            # the same driver without the HDF5 writers, for runs at BASELINE-config size where every writeOutput()
            # would compress about 1 GB of fluid fields (examples/pipe/run_reference_pipeflow_config3.py)
            jobs.append(base + ["-o", path(name + "_nohdf5")] + link)
    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as pool:   # one g++ each; a failure raises here
        list(pool.map(subprocess.check_call, jobs))


if __name__ == "__main__":
    build()
