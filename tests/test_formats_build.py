"""The second HIP extension is part of the build: after __graft_entry__.build()
the _gpuprobe_formats shared object exists and imports, and build_hip() still
returns the _gpuprobe path and rebuilds an output older than the shared
header. Needs no GPU (hipcc cross-compiles)."""
import os
import subprocess
import sys
import sysconfig

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "kata_xpu_device_plugin_amd")
EXT = sysconfig.get_config_var("EXT_SUFFIX")


def test_build_makes_and_imports_the_formats_extension():
    out = subprocess.run(
        [sys.executable, "-c",
         "import sys; sys.path.insert(0, %r); "
         "import __graft_entry__ as g; g.build(); "
         "from kata_xpu_device_plugin_amd import _gpuprobe_formats as f; "
         "print('entry points:', sorted(n for n in dir(f) if n[0] != '_'))" % REPO],
        capture_output=True, text=True, timeout=900, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "build OK" in out.stdout
    assert "mfma_probe_formats" in out.stdout
    assert os.path.exists(os.path.join(PKG, f"_gpuprobe_formats{EXT}"))
    assert os.path.exists(os.path.join(PKG, f"_gpuprobe{EXT}"))


def test_build_hip_staleness_looks_at_the_header(monkeypatch):
    """With fresh outputs nothing is compiled; an output older than
    probes/probe_host.h is (both of them); the return value is _gpuprobe's."""
    sys.path.insert(0, REPO)
    try:
        import setup as project_setup
    finally:
        sys.path.remove(REPO)
    assert set(project_setup.HIP_EXTENSIONS) == {"_gpuprobe", "_gpuprobe_formats"}
    outs = {m: os.path.join(PKG, f"{m}{EXT}") for m in project_setup.HIP_EXTENSIONS}
    assert all(os.path.exists(o) for o in outs.values()), "run build() first"
    header = os.path.join(REPO, "probes", "probe_host.h")
    sources = [os.path.join(REPO, "probes", s) for s in project_setup.HIP_EXTENSIONS.values()]
    newest_out = max(os.path.getmtime(o) for o in outs.values())
    oldest_out = min(os.path.getmtime(o) for o in outs.values())
    mtimes = {p: oldest_out - 200 for p in sources}
    real_getmtime = os.path.getmtime
    compiled = []
    monkeypatch.setattr(project_setup.subprocess, "run",
                        lambda cmd, **kw: compiled.append(cmd[cmd.index("-o") + 1]))
    monkeypatch.setattr(project_setup.os.path, "getmtime",
                        lambda p: mtimes.get(p, real_getmtime(p)))

    mtimes[header] = oldest_out - 100          # everything older than the outputs
    assert project_setup.build_hip(verbose=False) == outs["_gpuprobe"]
    assert compiled == []
    mtimes[header] = newest_out + 100          # header newer than both outputs
    assert project_setup.build_hip(verbose=False) == outs["_gpuprobe"]
    assert sorted(compiled) == sorted(outs.values())
    compiled.clear()
    mtimes[header] = oldest_out - 100
    mtimes[sources[1]] = newest_out + 100      # only the formats source is newer
    project_setup.build_hip(verbose=False)
    assert compiled == [outs["_gpuprobe_formats"]]
