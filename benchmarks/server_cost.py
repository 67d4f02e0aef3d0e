#!/usr/bin/env python3
"""Daemon cost per RPC: CPU µs and wall µs, Allocate vs a no-op RPC.

Starts the daemon the way bench.py does (mock 8-GPU node, kubelet stub,
the production CLI as its own process, default config), then drives a
fixed number of RPCs from ONE synchronous client and reads the daemon's
utime+stime from /proc/<pid>/stat before and after each batch. The
daemon's CPU time per RPC is the server-side cost that a queue of
concurrent clients multiplies; wall µs per RPC is what the single client
sees. One JSON line on stdout.

    python benchmarks/server_cost.py [--rpcs 20000] [--grpc-server aio]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def cpu_seconds(pid: int) -> float:
    with open(f"/proc/{pid}/stat") as f:
        fields = f.read().rsplit(")", 1)[1].split()
    return (int(fields[11]) + int(fields[12])) / os.sysconf("SC_CLK_TCK")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rpcs", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=2000)
    ap.add_argument("--grpc-server", default=None,
                    help="force KXDP_GRPC_SERVER for the daemon")
    args = ap.parse_args()

    import grpc

    from kata_xpu_device_plugin_amd.plugin import api
    from kata_xpu_device_plugin_amd.testing.kubelet_stub import KubeletStub
    from kata_xpu_device_plugin_amd.testing.mocknode import make_mock_node
    from kata_xpu_device_plugin_amd.utils.log import configure

    configure("WARNING")
    root = tempfile.mkdtemp(prefix="kxdp-cost-")
    node = make_mock_node(root, n_gpus=8)
    cfg = node.config()
    stub = KubeletStub(cfg.kubelet_socket_dir)
    stub.start()
    env = os.environ.copy()
    env.update({
        "KXDP_SYSFS_ROOT": cfg.sysfs_root,
        "KXDP_DEV_ROOT": cfg.dev_root,
        "KXDP_CDI_DIR": cfg.cdi_dir,
        "KXDP_KUBELET_DIR": cfg.kubelet_socket_dir,
        "KXDP_TOPOLOGY_HINT": cfg.topology_hint_path,
        "KXDP_PCI_IDS": "",
        "KXDP_AMDSMI_HEALTH": "0",
        "KXDP_LOG_LEVEL": "WARNING",
    })
    if args.grpc_server:
        env["KXDP_GRPC_SERVER"] = args.grpc_server
    daemon = subprocess.Popen(
        [sys.executable, "-m", "kata_xpu_device_plugin_amd"], env=env)
    try:
        reg = stub.wait_for_registration(1, timeout=30)[0]
        channel = grpc.insecure_channel(
            f"unix://{os.path.join(cfg.kubelet_socket_dir, reg.endpoint)}",
            options=[("grpc.optimization_target", "latency")])
        grpc.channel_ready_future(channel).result(timeout=10)
        plugin = api.DevicePluginStub(channel)
        alloc = api.AllocateRequest(container_requests=[
            api.ContainerAllocateRequest(devices_ids=["70"])])
        empty = api.Empty()

        def batch(call, arg, n):
            for _ in range(args.warmup):
                call(arg)
            c0, t0 = cpu_seconds(daemon.pid), time.perf_counter()
            for _ in range(n):
                call(arg)
            t1, c1 = time.perf_counter(), cpu_seconds(daemon.pid)
            return {"daemon_cpu_us_per_rpc": round((c1 - c0) / n * 1e6, 2),
                    "wall_us_per_rpc": round((t1 - t0) / n * 1e6, 2)}

        out = {
            "rpcs": args.rpcs,
            "grpc_server": args.grpc_server or "default",
            "allocate": batch(plugin.Allocate, alloc, args.rpcs),
            "noop": batch(plugin.GetDevicePluginOptions, empty, args.rpcs),
            # /proc tick resolution, spread over the batch
            "cpu_resolution_us_per_rpc": round(
                1e6 / os.sysconf("SC_CLK_TCK") / args.rpcs, 3),
        }
        print(json.dumps(out))
        channel.close()
    finally:
        daemon.terminate()
        try:
            daemon.wait(timeout=10)
        except subprocess.TimeoutExpired:
            daemon.kill()
        stub.stop()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
