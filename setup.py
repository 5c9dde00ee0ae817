"""Build the machin_amd gfx950 HIP extension in-tree.

    python setup.py build_ext --inplace

Drives hipcc DIRECTLY (no torch-hipify pass): every source in
machin_amd/ops/hip is already written against the native HIP API
(masquerading-as-CUDA device layer), so the tree carries zero
generated files. Produces machin_amd/ops/_machin_hip*.so next to the
package sources so the built artifact travels with any snapshot of
the repo.
"""
import multiprocessing.pool
import os
import subprocess
import sys
import sysconfig

from setuptools import Command, setup

ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")
HIP_DIR = os.path.join("machin_amd", "ops", "hip")
SOURCES = [
    "bindings.cpp",
    "sumtree.hip",
    "scans.hip",
    "projection.hip",
    "c51_loss.hip",
    "noisy_linear.hip",
    "multi_tensor.hip",
    "distributions.hip",
    "elementwise.hip",
    "framestack.hip",
    "framestack_vec.hip",
    "pixelcatch.hip",
    "conv1_wrw.hip",
    "bias_act.hip",
]


def _hipcc() -> str:
    rocm = os.environ.get("ROCM_HOME", os.environ.get("ROCM_PATH",
                                                      "/opt/rocm"))
    cand = os.path.join(rocm, "bin", "hipcc")
    return cand if os.path.exists(cand) else "hipcc"


class BuildHipExt(Command):
    """Compile + link the extension with hipcc, incrementally."""

    user_options = [("inplace", "i", "build in the source tree")]

    def initialize_options(self):
        self.inplace = True

    def finalize_options(self):
        pass

    def run(self):
        import torch
        from torch.utils.cpp_extension import (
            COMMON_HIP_FLAGS,
            include_paths,
            library_paths,
        )

        ext_suffix = sysconfig.get_config_var("EXT_SUFFIX") or ".so"
        out_so = os.path.join("machin_amd", "ops",
                              f"_machin_hip{ext_suffix}")
        obj_dir = os.path.join("build", f"hip_{ARCH}")
        os.makedirs(obj_dir, exist_ok=True)

        includes = include_paths("cuda") + [
            sysconfig.get_paths()["include"]
        ]
        defines = [
            "-DTORCH_EXTENSION_NAME=_machin_hip",
            "-DTORCH_API_INCLUDE_EXTENSION_H",
            "-D__HIP_PLATFORM_AMD__=1",
            f"-D_GLIBCXX_USE_CXX11_ABI="
            f"{int(torch._C._GLIBCXX_USE_CXX11_ABI)}",
            f"-DPYBIND11_COMPILER_TYPE=\"_gcc\"",
            f"-DPYBIND11_STDLIB=\"_libstdcpp\"",
            f"-DPYBIND11_BUILD_ABI=\"_cxxabi1011\"",
        ] + [f for f in COMMON_HIP_FLAGS if f.startswith("-D")]
        cflags = [
            "-O3", "-std=c++17", "-fPIC",
            f"--offload-arch={ARCH}",
            "-fno-gpu-rdc",
            "-Wno-unused-result",
        ]
        hipcc = _hipcc()

        def compile_one(src_name):
            src = os.path.join(HIP_DIR, src_name)
            obj = os.path.join(
                obj_dir, os.path.splitext(src_name)[0] + ".o"
            )
            deps = [src, os.path.join(HIP_DIR, "common.h"), __file__]
            if os.path.exists(obj) and all(
                os.path.getmtime(obj) >= os.path.getmtime(d)
                for d in deps
            ):
                return obj
            # bindings.cpp is host-only code (no kernels): hipcc
            # compiles it as plain C++ against the HIP runtime headers
            cmd = (
                [hipcc, "-c", src, "-o", obj]
                + cflags + defines
                + [f"-I{p}" for p in includes]
            )
            print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
            return obj

        with multiprocessing.pool.ThreadPool(
            min(len(SOURCES), os.cpu_count() or 4)
        ) as pool:
            objs = pool.map(compile_one, SOURCES)

        lib_dirs = library_paths("cuda")
        link = (
            [hipcc, "-shared", "-fPIC", "-o", out_so]
            + objs
            + [f"-L{p}" for p in lib_dirs]
            + [f"-Wl,-rpath,{p}" for p in lib_dirs]
            + [
                "-ltorch", "-ltorch_cpu", "-ltorch_hip", "-lc10",
                "-lc10_hip", "-ltorch_python", "-lamdhip64",
            ]
        )
        print(" ".join(link), flush=True)
        subprocess.check_call(link)
        print(f"built {out_so}", flush=True)


if __name__ == "__main__" and "build_ext" in sys.argv:
    # bypass setuptools' extension machinery entirely
    BuildHipExt(__import__("setuptools").dist.Distribution()).run()
    sys.exit(0)

setup(
    name="machin_amd",
    version="0.2.0",
    packages=[
        "machin_amd",
        "machin_amd.frame",
        "machin_amd.frame.buffers",
        "machin_amd.frame.algorithms",
        "machin_amd.frame.noise",
        "machin_amd.model",
        "machin_amd.model.nets",
        "machin_amd.model.algorithms",
        "machin_amd.parallel",
        "machin_amd.parallel.distributed",
        "machin_amd.parallel.server",
        "machin_amd.env",
        "machin_amd.env.wrappers",
        "machin_amd.env.envs",
        "machin_amd.auto",
        "machin_amd.utils",
        "machin_amd.ops",
    ],
)
