"""In-tree build of the native extensions.

* ``kata_xpu_device_plugin_amd._native`` — C++ fast paths (g++; runs on any
  Linux node, no GPU/ROCm needed).
* ``kata_xpu_device_plugin_amd._gpuprobe`` and ``._gpuprobe_formats`` — HIP
  gfx950 health probes (the second: FP64 / FP16 / INT8 / 2:4-sparse matrix
  cores), compiled by hipcc (cross-compiles fine on GPU-less builders). Built by
  ``build_hip()`` below / __graft_entry__.build(), not by setuptools, so a
  missing ROCm toolchain never breaks the control-plane build.

Usage: python setup.py build_ext --inplace && python -c "from setup import build_hip; build_hip()"
"""
import os
import subprocess
import sys

import pybind11

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = "kata_xpu_device_plugin_amd"


# HIP extension module → its source under probes/. Both include the headers
# there (probes/*.h: probe_host.h, mfma_forms.h).
HIP_EXTENSIONS = {
    "_gpuprobe": "xpu_probe.hip",
    "_gpuprobe_formats": "xpu_probe_formats.hip",
}


def build_hip(arch: str = "gfx950", verbose: bool = True) -> str:
    """Compile probes/xpu_probe.hip → kata_xpu_device_plugin_amd/_gpuprobe.so
    and probes/xpu_probe_formats.hip → …/_gpuprobe_formats.so with the same
    flags; returns the _gpuprobe path. An output newer than its source and
    every header under probes/ is kept."""
    import glob
    import sysconfig

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    headers = glob.glob(os.path.join(ROOT, "probes", "*.h"))
    ext = sysconfig.get_config_var("EXT_SUFFIX") or ".so"
    outs = {}
    for mod, name in HIP_EXTENSIONS.items():
        src = os.path.join(ROOT, "probes", name)
        out = outs[mod] = os.path.join(ROOT, PKG, f"{mod}{ext}")
        newest = max(os.path.getmtime(p) for p in [src, *headers])
        if os.path.exists(out) and os.path.getmtime(out) > newest:
            continue
        cmd = [
            hipcc, f"--offload-arch={arch}", "-O3", "-std=c++17",
            "-fPIC", "-shared",
            "-x", "hip", src,
            f"-I{pybind11.get_include()}",
            f"-I{sysconfig.get_paths()['include']}",
            "-o", out,
        ]
        if verbose:
            print("+", " ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)
    return outs["_gpuprobe"]


if __name__ == "__main__" or "setuptools" in sys.modules:
    from setuptools import Extension, setup

    if __name__ == "__main__":
        setup(
            name="kata-xpu-device-plugin-amd",
            version="0.1.0",
            packages=[
                PKG, f"{PKG}.discovery", f"{PKG}.topology", f"{PKG}.cdi",
                f"{PKG}.plugin", f"{PKG}.health", f"{PKG}.utils",
                f"{PKG}.testing", f"{PKG}.tools",
            ],
            # pinned pci.ids snapshot: deterministic naming on air-gapped
            # nodes (first entry of config.pci_ids_paths)
            package_data={PKG: ["data/pci.ids"]},
            include_package_data=True,
            entry_points={
                "console_scripts": [
                    "kata-xpu-device-plugin-amd=kata_xpu_device_plugin_amd.plugin.manager:main",
                    "kxdp-topo=kata_xpu_device_plugin_amd.tools.topo:main",
                    "kxdp-burnin=kata_xpu_device_plugin_amd.tools.burnin:main",
                    "kxdp-bind=kata_xpu_device_plugin_amd.tools.bind:main",
                    "kxdp-sriov=kata_xpu_device_plugin_amd.tools.sriov:main",
                    "kxdp-validate=kata_xpu_device_plugin_amd.tools.validate:main",
                    "kxdp-ident=kata_xpu_device_plugin_amd.tools.ident:main",
                    "kxdp-doctor=kata_xpu_device_plugin_amd.tools.doctor:main",
                    "kxdp-assignments=kata_xpu_device_plugin_amd.tools.assignments:main",
                    "kxdp-resourceslice=kata_xpu_device_plugin_amd.tools.resourceslice:main",
                    "kxdp-partition=kata_xpu_device_plugin_amd.tools.partition:main",
                ],
            },
            ext_modules=[
                Extension(
                    f"{PKG}._native",
                    sources=["native/xpu_native.cpp",
                             "native/xpu_grpc_server.cpp"],
                    depends=["native/h2.h", "native/hpack.h",
                             "native/pbwire.h"],
                    include_dirs=[pybind11.get_include(), "native"],
                    extra_compile_args=["-O2", "-std=c++17"],
                    extra_link_args=["-pthread"],
                    language="c++",
                ),
            ],
        )
