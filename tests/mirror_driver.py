"""tests/cpp/host_mirror_driver.cpp compiled once a test session, for every test module that runs it"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "host_mirror_driver.cpp")
_EXE = None


def host_mirror_driver(tmp_path_factory):
    global _EXE
    if _EXE is None or not os.path.exists(_EXE):
        from auncel_amd import build
        build.build_host()
        exe = str(tmp_path_factory.mktemp("drv") / "host_mirror_driver")
        subprocess.run(["g++", "-std=c++17", "-O1", DRIVER_SRC, "-o", exe, "-L" + build.LIBDIR, "-lfaiss_amd", "-launcel_amd",
                        "-Wl,-rpath," + build.LIBDIR, "-pthread"], check=True)
        _EXE = exe
    return _EXE
