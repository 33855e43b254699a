"""Build libgangfit.so (HIP kernels + C ABI) in-tree for gfx950 with hipcc.  No JIT cache: the .so sits next to the
package so that it travels with the repository snapshot to the GPU box."""
from __future__ import annotations

import glob
import os
import shutil
import subprocess

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # k8s-spark-scheduler_amd/
_REPO_ROOT = os.path.dirname(_PKG_ROOT)
CSRC = os.path.join(_PKG_ROOT, "csrc")
LIB_PATH = os.path.join(_PKG_ROOT, "libgangfit.so")
HOST_LIB_PATH = os.path.join(_PKG_ROOT, "libgangfit_host.so")
HOST_BENCH_PATH = os.path.join(_PKG_ROOT, "host_bench")  # end-to-end Filter timing through the host mirror
HOST_TEST_PATH = os.path.join(_PKG_ROOT, "host_test")  # C++ tests of the host mirror (host/tests/host_test.cpp)
HOST_OVERHEAD_TEST_PATH = os.path.join(_PKG_ROOT, "host_overhead_test")  # ... of its flat route with overhead (host_overhead_test.cpp)
HOST_CLUSTER_SCAN_TEST_PATH = os.path.join(_PKG_ROOT, "host_cluster_scan_test")  # ... of the resident capacity scan (host_cluster_scan_test.cpp)
HOST_CLUSTER_SCAN_SETS_TEST_PATH = os.path.join(_PKG_ROOT, "host_cluster_scan_sets_test")  # ... of the all-groups scan (host_cluster_scan_sets_test.cpp)
HOST_SNAPSHOT_LABELS_TEST_PATH = os.path.join(_PKG_ROOT, "host_snapshot_labels_test")  # ... of builds with a prioritized label (host_snapshot_labels_test.cpp)
HOST_EXECUTOR_RESIDENT_TEST_PATH = os.path.join(_PKG_ROOT, "host_executor_resident_test")  # ... of the resident executor Filter (host_executor_resident_test.cpp)
HOST_GROUP_FILTER_TEST_PATH = os.path.join(_PKG_ROOT, "host_group_filter_test")  # ... of the driver Filters of several groups (host_group_filter_test.cpp)
HOST_FILTER_EFFICIENCY_TEST_PATH = os.path.join(_PKG_ROOT, "host_filter_efficiency_test")  # ... of the Filters' packing efficiency (host_filter_efficiency_test.cpp)
HOST_CLUSTER_FIND_NODES_TEST_PATH = os.path.join(_PKG_ROOT, "host_cluster_find_nodes_test")  # ... of the resident failover reconcile (host_cluster_find_nodes_test.cpp)
HOST_CLUSTER_UPDATE_TEST_PATH = os.path.join(_PKG_ROOT, "host_cluster_update_test")  # ... of node rows changed in place (host_cluster_update_test.cpp)
INCLUDE = os.path.join(_REPO_ROOT, "include")

_SOURCES = ["gangfit_kernels.hip", "gangfit_snapshot.hip", "gangfit_api.cpp", "gangfit_api_snapshot.cpp", "gangfit_api_fit.cpp",
            "gangfit_api_worker.cpp", "gangfit_api_group.cpp", "gangfit_api_scan.cpp", "gangfit_api_eff.cpp"]
_HEADERS = [os.path.join(CSRC, "gangfit_device.h"), os.path.join(CSRC, "gangfit_slot_layout.h"), os.path.join(CSRC, "gangfit_label_plan.h"),
            os.path.join(CSRC, "gangfit_worker_rounds.h"), os.path.join(CSRC, "gangfit_worker_rows.h"),
            os.path.join(CSRC, "gangfit_chain_lds.h"),
            os.path.join(INCLUDE, "gangfit.h")]


def hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: libgangfit cannot be built (ROCm toolchain required)")
    return exe


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_native(force: bool = False) -> str:
    """hipcc --offload-arch=gfx950 ... -> k8s-spark-scheduler_amd/libgangfit.so.  The translation units are compiled side by side
    (one hipcc process each: the two kernel files take most of a minute, the seven host files a few seconds), then linked."""
    srcs = [os.path.join(CSRC, s) for s in _SOURCES]
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + _HEADERS  # .inc files are #included by the .hip
    if force or _stale(LIB_PATH, deps):
        import tempfile
        from concurrent.futures import ThreadPoolExecutor

        common = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", INCLUDE, "-I", CSRC]
        with tempfile.TemporaryDirectory(prefix="gangfit_build_") as tmp:
            objs = [os.path.join(tmp, os.path.basename(s) + ".o") for s in srcs]

            def one(pair):
                subprocess.check_call([*common, "-c", pair[0], "-o", pair[1]])

            with ThreadPoolExecutor(max_workers=len(srcs)) as pool:
                list(pool.map(one, zip(srcs, objs)))
            subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", LIB_PATH])
    return LIB_PATH


def build_host(force: bool = False) -> str:
    """C++ host mirror of the reference's plug-in interface (string node names, Quantity parsing) on top of the C ABI."""
    host_dir = os.path.join(_PKG_ROOT, "host")
    if not os.path.isdir(host_dir):
        return ""
    srcs = [os.path.join(host_dir, f) for f in sorted(os.listdir(host_dir)) if f.endswith(".cpp")]
    hdrs = [os.path.join(host_dir, f) for f in sorted(os.listdir(host_dir)) if f.endswith(".hpp")]
    if not srcs:
        return ""
    if force or _stale(HOST_LIB_PATH, srcs + hdrs + _HEADERS + [LIB_PATH]):
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", INCLUDE, "-I", host_dir, *srcs,
               "-L", _PKG_ROOT, "-lgangfit", "-Wl,-rpath,$ORIGIN", "-o", HOST_LIB_PATH]
        subprocess.check_call(cmd)
    # the programs on top of the library: (source under host/tests/, output, flags); the tests run threads, host_bench is timed
    test_flags, bench_flags = ["-O1", "-std=c++17", "-Wall", "-pthread"], ["-O2", "-std=c++17", "-Wall"]
    programs = [("host_test.cpp", HOST_TEST_PATH, test_flags),
                ("host_overhead_test.cpp", HOST_OVERHEAD_TEST_PATH, test_flags),
                ("host_cluster_scan_test.cpp", HOST_CLUSTER_SCAN_TEST_PATH, test_flags),
                ("host_cluster_scan_sets_test.cpp", HOST_CLUSTER_SCAN_SETS_TEST_PATH, test_flags),
                ("host_snapshot_labels_test.cpp", HOST_SNAPSHOT_LABELS_TEST_PATH, test_flags),
                ("host_executor_resident_test.cpp", HOST_EXECUTOR_RESIDENT_TEST_PATH, test_flags),
                ("host_group_filter_test.cpp", HOST_GROUP_FILTER_TEST_PATH, test_flags),
                ("host_filter_efficiency_test.cpp", HOST_FILTER_EFFICIENCY_TEST_PATH, test_flags),
                ("host_cluster_find_nodes_test.cpp", HOST_CLUSTER_FIND_NODES_TEST_PATH, test_flags),
                ("host_cluster_update_test.cpp", HOST_CLUSTER_UPDATE_TEST_PATH, test_flags),
                ("host_bench.cpp", HOST_BENCH_PATH, bench_flags)]
    tests_dir = os.path.join(host_dir, "tests")
    test_hdrs = glob.glob(os.path.join(tests_dir, "*.hpp"))  # what the test programs share
    for name, out, flags in programs:
        src = os.path.join(tests_dir, name)
        if os.path.exists(src) and (force or _stale(out, [src, HOST_LIB_PATH] + hdrs + test_hdrs)):
            subprocess.check_call(["g++", *flags, "-I", INCLUDE, "-I", host_dir, src, "-L", _PKG_ROOT, "-lgangfit_host", "-lgangfit",
                                   "-Wl,-rpath,$ORIGIN", "-o", out])
    return HOST_LIB_PATH


if __name__ == "__main__":
    print(build_native(force=True))
    print(build_host(force=True))
