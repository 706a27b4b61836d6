"""The source files of the GPU-free host library, as vi_slam_amd/csrc/Makefile lists them (HOST_SRCS): for the tests that
compile the host logic into a program of their own instead of loading libvslam_host.so."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vi_slam_amd", "csrc")


def host_sources():
    """absolute paths, in the Makefile's order"""
    names = subprocess.check_output(["make", "-s", "--no-print-directory", "-C", CSRC, "print-host-srcs"], text=True).split()
    assert names and all(n.endswith(".cpp") for n in names), names
    return [os.path.join(CSRC, n) for n in names]
