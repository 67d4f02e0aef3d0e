"""Native gRPC server (native/xpu_grpc_server.cpp, h2.h, hpack.h).

* the stand-alone protocol self-test, compiled with plain g++;
* parity of every Allocate outcome between the native and the grpc.aio
  flavour (same parsed message, same deterministic bytes, same status code
  and message);
* a raw-frame HTTP/2 client (plain ``socket``) standing in for the wire
  behaviour of kubelet's grpc-go that the Python grpc client never shows:
  Huffman-coded and dynamic-table-indexed headers, CONTINUATION, padding,
  split DATA, interleaved streams, small flow-control windows;
* ListAndWatch fan-out and shutdown, concurrency and counters.
"""
import os
import shutil
import socket
import struct
import subprocess
import threading
import time

import grpc
import pytest

from kata_xpu_device_plugin_amd.plugin import api
from kata_xpu_device_plugin_amd.plugin.manager import PluginManager
from kata_xpu_device_plugin_amd.plugin.server import native_server_available
from kata_xpu_device_plugin_amd.testing.mocknode import MockGPU, make_mock_node

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = "/v1beta1.DevicePlugin/"


def test_extension_provides_server():
    assert native_server_available()


def test_h2_selftest_plain_gpp(tmp_path):
    """HPACK vectors, Kraft sum, dynamic-table eviction, frame parsing and
    the fixed-seed fuzz — no Python, no sanitizer (that is `make
    h2-selftest-asan`)."""
    exe = str(tmp_path / "h2_selftest")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "native"),
         os.path.join(ROOT, "native", "tests", "h2_selftest.cpp"), "-o", exe],
        check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
class Served:
    def __init__(self, root, flavour, build=None, **cfg_overrides):
        self.node = make_mock_node(str(root), n_gpus=2)
        if build:
            build(self.node)
        self.cfg = self.node.config(grpc_server=flavour, **cfg_overrides)
        self.mgr = PluginManager(self.cfg)
        self.mgr.setup()
        self.mgr.start(register=False)
        self._channels = []

    def plugin(self, gid="70"):
        for p in self.mgr.plugins.values():
            if p.state.device(gid) is not None:
                return p
        raise KeyError(gid)

    def stub(self, gid="70"):
        ch = grpc.insecure_channel(f"unix://{self.plugin(gid).socket_path}")
        grpc.channel_ready_future(ch).result(timeout=5)
        self._channels.append(ch)
        return api.DevicePluginStub(ch)

    def close(self):
        for ch in self._channels:
            ch.close()
        self.mgr.stop()
        shutil.rmtree(self.cfg.kubelet_socket_dir, ignore_errors=True)


@pytest.fixture
def native(tmp_path):
    s = Served(tmp_path, "native")
    assert s.plugin()._native_server is not None
    yield s
    s.close()


def _alloc_req(*containers):
    return api.AllocateRequest(container_requests=[
        api.ContainerAllocateRequest(devices_ids=list(ids)) for ids in containers])


def _outcome(served, gid, request):
    try:
        resp = served.stub(gid).Allocate(request, timeout=5)
    except grpc.RpcError as e:
        return ("error", e.code(), e.details())
    return ("ok", resp, resp.SerializeToString(deterministic=True))


# ---------------------------------------------------------------------------
# parity native vs aio
# ---------------------------------------------------------------------------
def _vf_node(node):
    node.add_gpu(MockGPU(bdf="0000:0a:02.0", device_id=0x75B3,
                         iommu_group="200", physfn_bdf="0000:0a:00.0"))


def _audio_node(node):
    # group 70 gets a second (audio) function: a multi-function group
    bdf = "0000:0a:00.1"
    d = node._pci_dir(bdf)
    node._write(os.path.join(d, "vendor"), "0x1002\n")
    node._write(os.path.join(d, "device"), "0xab30\n")
    node._write(os.path.join(d, "class"), "0x040300\n")
    node._write(os.path.join(d, "numa_node"), "0\n")
    node._symlink(os.path.join(node.sysfs, "bus", "pci", "drivers", "vfio-pci"),
                  os.path.join(d, "driver"))
    node._symlink(os.path.join(node.sysfs, "kernel", "iommu_groups", "70"),
                  os.path.join(d, "iommu_group"))


def _pci(served, bdf):
    return served.node._pci_dir(bdf)


def _vanish(served):
    shutil.rmtree(_pci(served, "0000:12:00.0"))


def _wrong_driver(served):
    link = os.path.join(_pci(served, "0000:12:00.0"), "driver")
    os.unlink(link)
    target = os.path.join(served.node.sysfs, "bus", "pci", "drivers", "amdgpu")
    os.makedirs(target, exist_ok=True)
    os.symlink(target, link)


def _wrong_vendor(served):
    with open(os.path.join(_pci(served, "0000:12:00.0"), "vendor"), "w") as f:
        f.write("0x10de\n")


def _unhealthy(served):
    assert served.plugin().state.set_health("71", False, source="test")


PARITY_CASES = {
    # name: (cfg overrides, node builder, device id that picks the plugin,
    #        request, mutation after start)
    "cdi-cri": ({}, None, "70", _alloc_req(["70", "71"]), None),
    "cdi-annotations": ({"device_list_strategy": "cdi-annotations"}, None,
                        "70", _alloc_req(["71", "70"]), None),
    "device-nodes": ({"device_list_strategy": "device-nodes"}, None, "70",
                     _alloc_req(["70", "71"]), None),
    "device-nodes-empty": ({"device_list_strategy": "device-nodes"}, None,
                           "70", _alloc_req([]), None),
    "multi-function-group": ({}, _audio_node, "70", _alloc_req(["70"]), None),
    "sriov-vf": ({}, _vf_node, "200", _alloc_req(["200"]), None),
    "two-containers": ({}, None, "70", _alloc_req(["70"], ["71"]), None),
    "empty-request": ({}, None, "70", api.AllocateRequest(), None),
    "empty-container": ({}, None, "70", _alloc_req([]), None),
    "unknown-id": ({}, None, "70", _alloc_req(["70", "99"]), None),
    "unhealthy": ({}, None, "70", _alloc_req(["71"]), _unhealthy),
    "vanished-bdf": ({}, None, "70", _alloc_req(["70", "71"]), _vanish),
    "wrong-driver": ({}, None, "70", _alloc_req(["71"]), _wrong_driver),
    "wrong-vendor": ({}, None, "70", _alloc_req(["71"]), _wrong_vendor),
}
EXPECT_ERROR = {"unknown-id", "unhealthy", "vanished-bdf", "wrong-driver",
                "wrong-vendor"}


@pytest.mark.parametrize("case", sorted(PARITY_CASES))
def test_allocate_parity_native_vs_aio(tmp_path, case):
    overrides, build, gid, request, mutate = PARITY_CASES[case]
    got = {}
    for flavour in ("native", "aio"):
        # same root for both, so the paths inside the responses agree
        s = Served(tmp_path / "node", flavour, build=build, **overrides)
        try:
            assert (s.plugin(gid)._native_server is not None) == (flavour == "native")
            if mutate:
                mutate(s)
            got[flavour] = _outcome(s, gid, request)
            plugin = s.plugin(gid)
            counters = (plugin.allocations, plugin.allocate_failures)
        finally:
            s.close()
            shutil.rmtree(tmp_path / "node")
        assert counters == ((0, 1) if case in EXPECT_ERROR else (1, 0))
    n, a = got["native"], got["aio"]
    assert n[0] == a[0] == ("error" if case in EXPECT_ERROR else "ok")
    if n[0] == "error":
        assert n[1] == a[1] == grpc.StatusCode.INVALID_ARGUMENT
        assert n[2] == a[2] and n[2]
    else:
        assert n[1] == a[1]          # parsed messages
        assert n[2] == a[2]          # deterministic bytes
        if case not in ("empty-request",):
            assert len(n[1].container_responses) == len(request.container_requests)


def test_state_change_visible_to_next_allocate(native):
    """set_health()/replace_devices() push the table synchronously."""
    ps = native.stub()
    state = native.plugin().state
    for _ in range(20):
        state.set_health("70", False, source="t")
        with pytest.raises(grpc.RpcError) as e:
            ps.Allocate(_alloc_req(["70"]))
        assert e.value.details() == "device 70 is Unhealthy"
        state.set_health("70", True, source="t")
        assert ps.Allocate(_alloc_req(["70"])).container_responses[0].cdi_devices
    only_71 = {"71": state.device("71")}
    both = {g: state.device(g) for g in ("70", "71")}
    state.replace_devices(only_71)
    with pytest.raises(grpc.RpcError) as e:
        ps.Allocate(_alloc_req(["70"]))
    assert e.value.details() == "unknown device id 70"
    state.replace_devices(both)
    ps.Allocate(_alloc_req(["70"]))


def test_other_rpcs_and_unknown_method(native):
    ps = native.stub()
    opts = ps.GetDevicePluginOptions(api.Empty())
    assert opts.get_preferred_allocation_available and not opts.pre_start_required
    ps.PreStartContainer(api.PreStartContainerRequest(devices_ids=["70"]))
    pref = ps.GetPreferredAllocation(api.PreferredAllocationRequest(
        container_requests=[api.ContainerPreferredAllocationRequest(
            available_device_ids=["70", "71"], allocation_size=1)]))
    assert len(pref.container_responses[0].device_ids) == 1
    ch = grpc.insecure_channel(f"unix://{native.plugin().socket_path}")
    try:
        with pytest.raises(grpc.RpcError) as e:
            ch.unary_unary(P + "Nope")(b"", timeout=5)
        assert e.value.code() == grpc.StatusCode.UNIMPLEMENTED
    finally:
        ch.close()


def test_flavour_switch_fails_loudly(tmp_path, monkeypatch):
    from kata_xpu_device_plugin_amd.plugin import server as server_mod
    s = Served(tmp_path, "aio")
    try:
        plugin = s.plugin()
        assert plugin._native_server is None
        plugin.cfg.grpc_server = "native"
        monkeypatch.setattr(server_mod, "_NATIVE", None)
        with pytest.raises(RuntimeError):
            plugin._use_native_server()
        plugin.cfg.grpc_server = "auto"
        assert plugin._use_native_server() is False
        plugin.cfg.native = "require"
        with pytest.raises(RuntimeError):
            plugin._use_native_server()
    finally:
        s.close()


# ---------------------------------------------------------------------------
# raw-frame client
# ---------------------------------------------------------------------------
DATA, HEADERS, PRIORITY, RST_STREAM, SETTINGS, PUSH_PROMISE, PING, GOAWAY, \
    WINDOW_UPDATE, CONTINUATION = range(10)
END_STREAM, END_HEADERS, PADDED, ACK = 0x1, 0x4, 0x8, 0x1
PREFACE = b"PRI * HTTP/2.0\r\n\r\nSM\r\n\r\n"

# Huffman-coded strings as produced by an independent HPACK encoder
# (nghttp2) for these exact values.
HUFF = {
    P + "Allocate": bytes.fromhex("63b8632a4615ef97b9885d745b31aa621a28390692ff"),
    P + "ListAndWatch": bytes.fromhex(
        "63b8632a4615ef97b9885d745b31aa633990986a9390d249ff"),
    P + "GetDevicePluginOptions": bytes.fromhex(
        "63b8632a4615ef97b9885d745b31aa6311537cbdcc42eba2d98d56aad263d48f"),
    "application/grpc": bytes.fromhex("1d75d0620d263d4c4d6564"),
    "trailers": bytes.fromhex("4d833505b11f"),
}


def _hstr(raw, huffman):
    body = HUFF[raw] if huffman else raw.encode()
    assert len(body) < 127
    return bytes([len(body) | (0x80 if huffman else 0)]) + body


def block_indexing(path):
    """grpc-go style: :method POST, :scheme http indexed; :path,
    content-type and te as Huffman literals WITH incremental indexing —
    they enter the dynamic table as entries 64, 63, 62."""
    return (b"\x83\x86" + b"\x44" + _hstr(path, True)
            + b"\x5f" + _hstr("application/grpc", True)
            + b"\x40\x02te" + _hstr("trailers", True))


BLOCK_REUSE = b"\x83\x86\xc0\xbf\xbe"   # the three dynamic entries again


def block_plain(path):
    """Literals without indexing, raw strings (what grpc-core sends)."""
    out = b"\x83\x86" + b"\x04" + _hstr(path, False)
    out += b"\x0f\x10" + _hstr("application/grpc", False)   # name index 31
    return out


def frame(ftype, flags, sid, payload=b""):
    return struct.pack(">I", len(payload))[1:] + bytes([ftype, flags]) + \
        struct.pack(">I", sid) + payload


def grpc_msg(payload, compressed=0):
    return bytes([compressed]) + struct.pack(">I", len(payload)) + payload


class RawClient:
    def __init__(self, path, settings=b"", preface=PREFACE):
        self.sock = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
        self.sock.settimeout(5)
        self.sock.connect(path)
        self.buf = b""
        self.frames = []
        self.sock.sendall(preface + frame(SETTINGS, 0, 0, settings))

    def send(self, data):
        self.sock.sendall(data)

    def _read_frame(self):
        while True:
            if len(self.buf) >= 9:
                n = int.from_bytes(self.buf[:3], "big")
                if len(self.buf) >= 9 + n:
                    f = (self.buf[3], self.buf[4],
                         int.from_bytes(self.buf[5:9], "big") & 0x7FFFFFFF,
                         self.buf[9:9 + n])
                    self.buf = self.buf[9 + n:]
                    return f
            chunk = self.sock.recv(65536)
            if not chunk:
                return None
            self.buf += chunk

    def wait(self, pred, what="frame"):
        """Read frames until pred(frame); returns it (all frames are kept)."""
        while True:
            f = self._read_frame()
            assert f is not None, f"connection closed waiting for {what}"
            self.frames.append(f)
            if pred(f):
                return f

    def wait_closed(self):
        while True:
            f = self._read_frame()
            if f is None:
                return
            self.frames.append(f)

    def unary(self, sid, block, payload):
        """Response message bytes and trailer block of one unary call whose
        request frames the caller has already sent."""
        self.wait(lambda f: f[0] == HEADERS and f[2] == sid and f[1] & END_STREAM,
                  f"trailers of stream {sid}")
        return self.stream_data(sid), self.trailers(sid)

    def stream_data(self, sid):
        return b"".join(f[3] for f in self.frames if f[0] == DATA and f[2] == sid)

    def trailers(self, sid):
        return [f[3] for f in self.frames
                if f[0] == HEADERS and f[2] == sid and f[1] & END_STREAM][-1]

    def close(self):
        self.sock.close()


def _status(trailer_block):
    """grpc-status from our server's literal (never-compressed) encoding."""
    i = trailer_block.index(b"grpc-status")
    n = trailer_block[i + 11]
    return int(trailer_block[i + 12:i + 12 + n])


def _allocate_ok(message_bytes, gid):
    assert message_bytes[0] == 0
    assert int.from_bytes(message_bytes[1:5], "big") == len(message_bytes) - 5
    resp = api.AllocateResponse.FromString(message_bytes[5:])
    assert [d.name for d in resp.container_responses[0].cdi_devices] == \
        [f"amd.com/gpu={gid}"]


REQ70 = _alloc_req(["70"]).SerializeToString()
REQ71 = _alloc_req(["71"]).SerializeToString()


def test_raw_huffman_dynamic_table_continuation_padding(native):
    c = RawClient(native.plugin().socket_path)
    try:
        # 1: Huffman :path, indexed into the dynamic table
        c.send(frame(HEADERS, END_HEADERS, 1, block_indexing(P + "Allocate"))
               + frame(DATA, END_STREAM, 1, grpc_msg(REQ70)))
        data, trailers = c.unary(1, None, None)
        _allocate_ok(data, "70")
        assert _status(trailers) == 0
        # 3: only references to the entries created by stream 1
        c.send(frame(HEADERS, END_HEADERS, 3, BLOCK_REUSE)
               + frame(DATA, END_STREAM, 3, grpc_msg(REQ71)))
        data, trailers = c.unary(3, None, None)
        _allocate_ok(data, "71")
        # 5: padded HEADERS + 2 × CONTINUATION, message one byte per DATA
        b = block_plain(P + "Allocate")
        first = bytes([4]) + b[:5] + b"\0" * 4
        c.send(frame(HEADERS, PADDED, 5, first)
               + frame(CONTINUATION, 0, 5, b[5:17])
               + frame(CONTINUATION, END_HEADERS, 5, b[17:]))
        msg = grpc_msg(REQ70)
        for i, byte in enumerate(msg):
            c.send(frame(DATA, END_STREAM if i == len(msg) - 1 else 0, 5,
                         bytes([byte])))
        data, trailers = c.unary(5, None, None)
        _allocate_ok(data, "70")
        # PING gets its ack with the same payload
        c.send(frame(PING, 0, 0, b"kxdpping"))
        ack = c.wait(lambda f: f[0] == PING)
        assert ack[1] & ACK and ack[3] == b"kxdpping"
    finally:
        c.close()


def test_raw_interleaved_streams_and_window_updates(native):
    """Two streams interleaved; then ~3000 Allocates (> 65 535 request bytes)
    on one connection: the server must keep granting connection window."""
    c = RawClient(native.plugin().socket_path)
    try:
        m70, m71 = grpc_msg(REQ70), grpc_msg(REQ71)
        c.send(frame(HEADERS, END_HEADERS, 1, block_plain(P + "Allocate"))
               + frame(HEADERS, END_HEADERS, 3, block_plain(P + "Allocate"))
               + frame(DATA, 0, 1, m70[:3]) + frame(DATA, 0, 3, m71[:6])
               + frame(DATA, 0, 1, m70[3:]) + frame(DATA, END_STREAM, 3, m71[6:])
               + frame(DATA, END_STREAM, 1, b""))
        c.wait(lambda f: f[0] == HEADERS and f[2] == 1 and f[1] & END_STREAM)
        if not any(f[0] == HEADERS and f[2] == 3 and f[1] & END_STREAM
                   for f in c.frames):
            c.wait(lambda f: f[0] == HEADERS and f[2] == 3 and f[1] & END_STREAM)
        _allocate_ok(c.stream_data(1), "70")
        _allocate_ok(c.stream_data(3), "71")
        c.frames.clear()

        block = block_plain(P + "Allocate")
        pad = grpc_msg(_alloc_req(["70"], *[[] for _ in range(8)]).SerializeToString())
        sent, sid, window = 0, 5, 65535 - len(m70) - len(m71)
        done = consumed = 0
        n_calls = 3000
        while done < n_calls:
            batch = b""
            batch_n = 0
            while sid < 5 + 2 * n_calls and batch_n < 50 and window >= len(pad):
                batch += frame(HEADERS, END_HEADERS, sid, block) + \
                    frame(DATA, END_STREAM, sid, pad)
                window -= len(pad)
                sent += len(pad)
                sid += 2
                batch_n += 1
            assert batch_n, "stalled: no connection window granted"
            c.send(batch)
            got = 0
            while got < batch_n:
                f = c.wait(lambda f: True)
                if f[0] == WINDOW_UPDATE and f[2] == 0:
                    window += int.from_bytes(f[3], "big")
                elif f[0] == DATA:
                    # our side of the bargain: without these the server's
                    # connection send window runs dry and it must queue
                    consumed += len(f[3])
                    if consumed >= 30000:
                        c.send(frame(WINDOW_UPDATE, 0, 0,
                                     struct.pack(">I", consumed)))
                        consumed = 0
                elif f[0] == HEADERS and f[1] & END_STREAM:
                    assert _status(f[3]) == 0
                    got += 1
            done += batch_n
            c.frames.clear()
        assert sent > 65535
        assert native.plugin().allocations == n_calls + 2
    finally:
        c.close()


def test_raw_small_window_list_and_watch_then_reset(native):
    """INITIAL_WINDOW_SIZE=16: the ListAndWatch message arrives only as
    WINDOW_UPDATEs are granted; RST_STREAM drops the stream and a unary on
    the same connection still completes."""
    expected = api.ListAndWatchResponse(
        devices=native.plugin()._device_list()).SerializeToString()
    c = RawClient(native.plugin().socket_path,
                  settings=struct.pack(">HI", 4, 16))
    try:
        c.wait(lambda f: f[0] == SETTINGS and f[1] & ACK)
        c.send(frame(HEADERS, END_HEADERS, 1, block_indexing(P + "ListAndWatch"))
               + frame(DATA, END_STREAM, 1, grpc_msg(b"")))
        c.wait(lambda f: f[0] == DATA and f[2] == 1)
        total = 5 + len(expected)
        assert total > 16
        grants = 0
        while len(c.stream_data(1)) < total:
            have = len(c.stream_data(1))
            assert have == min(total, 16 * (grants + 1)), "sent beyond the window"
            # nothing more may come until the window is opened
            c.sock.settimeout(0.05)
            with pytest.raises(socket.timeout):
                c.sock.recv(1)
            c.sock.settimeout(5)
            c.send(frame(WINDOW_UPDATE, 0, 1, struct.pack(">I", 16)))
            grants += 1
            want = min(total, 16 * (grants + 1))
            while len(c.stream_data(1)) < want:
                c.wait(lambda f: f[0] == DATA and f[2] == 1)
        assert c.stream_data(1) == grpc_msg(expected)
        assert all(len(f[3]) <= 16 for f in c.frames if f[0] == DATA)
        # reset the stream, then a unary (its response needs window too)
        c.send(frame(RST_STREAM, 0, 1, struct.pack(">I", 8)))
        c.send(frame(SETTINGS, 0, 0, struct.pack(">HI", 4, 65535)))
        c.send(frame(HEADERS, END_HEADERS, 3, block_plain(P + "GetDevicePluginOptions"))
               + frame(DATA, END_STREAM, 3, grpc_msg(b"")))
        data, trailers = c.unary(3, None, None)
        assert _status(trailers) == 0
        opts = api.DevicePluginOptions.FromString(data[5:])
        assert opts.get_preferred_allocation_available
        # the reset stream's subscription is gone
        deadline = time.time() + 5
        while native.plugin()._stream_subscriptions and time.time() < deadline:
            time.sleep(0.01)
        assert not native.plugin()._stream_subscriptions
    finally:
        c.close()


def _goaway_code(client):
    client.wait_closed()
    goaways = [f for f in client.frames if f[0] == GOAWAY]
    assert goaways, "connection closed without GOAWAY"
    return int.from_bytes(goaways[-1][3][4:8], "big")


def test_raw_malformed_input_gets_goaway_and_server_survives(native):
    path = native.plugin().socket_path
    c = RawClient(path, preface=b"GET / HTTP/1.1\r\nHost: x\r\n\r\n")
    assert _goaway_code(c) == 1            # PROTOCOL_ERROR
    c.close()
    c = RawClient(path)
    c.send(b"\x00\x40\x01" + bytes([DATA, 0]) + struct.pack(">I", 1))  # 16385
    assert _goaway_code(c) == 6            # FRAME_SIZE_ERROR
    c.close()
    c = RawClient(path)
    c.send(frame(CONTINUATION, END_HEADERS, 1, b""))
    assert _goaway_code(c) == 1
    c.close()
    c = RawClient(path)
    c.send(frame(HEADERS, END_HEADERS, 1, b"\xff\xff\xff\xff\xff\xff\xff"))
    assert _goaway_code(c) == 9            # COMPRESSION_ERROR
    c.close()
    # compressed flag: a status, not a connection error
    c = RawClient(path)
    try:
        c.send(frame(HEADERS, END_HEADERS, 1, block_plain(P + "Allocate"))
               + frame(DATA, END_STREAM, 1, grpc_msg(REQ70, compressed=1)))
        _, trailers = c.unary(1, None, None)
        assert _status(trailers) == 12
        c.send(frame(HEADERS, END_HEADERS, 3, block_plain(P + "Nope"))
               + frame(DATA, END_STREAM, 3, grpc_msg(b"")))
        _, trailers = c.unary(3, None, None)
        assert _status(trailers) == 12
        c.send(frame(HEADERS, END_HEADERS, 5, block_plain(P + "Allocate"))
               + frame(DATA, END_STREAM, 5, grpc_msg(REQ70)))
        data, _ = c.unary(5, None, None)
        _allocate_ok(data, "70")
    finally:
        c.close()
    # and a fresh ordinary client is served
    assert native.stub().Allocate(_alloc_req(["70"])).container_responses


# ---------------------------------------------------------------------------
# ListAndWatch
# ---------------------------------------------------------------------------
def _health(msg):
    return {d.id: d.health for d in msg.devices}


def test_list_and_watch_fanout_burst_and_stop(native):
    plugin = native.plugin()
    stubs = [native.stub(), native.stub()]          # two connections
    streams = [s.ListAndWatch(api.Empty()) for s in stubs for _ in range(3)]
    for st in streams:
        first = next(st)
        assert _health(first) == {"70": api.HEALTHY, "71": api.HEALTHY}
    assert len(plugin._stream_subscriptions) == 6
    # one change → one push on every stream
    plugin.state.set_health("70", False, source="t")
    for st in streams:
        assert _health(next(st))["70"] == api.UNHEALTHY
    # a burst ends with the newest state on every stream
    for i in range(40):
        plugin.state.set_health("71", i % 2 == 1, source="t")
    plugin.state.set_health("70", True, source="t")
    final = {"70": api.HEALTHY, "71": api.HEALTHY}
    for st in streams:
        seen = 0
        while True:
            seen += 1
            if _health(next(st)) == final:
                break
        assert seen <= 41
    # stop() ends the streams with OK (plain end of iteration)
    ends = []

    def drain(st):
        try:
            for _ in st:
                pass
            ends.append(grpc.StatusCode.OK)
        except grpc.RpcError as e:
            ends.append(e.code())

    threads = [threading.Thread(target=drain, args=(st,)) for st in streams]
    for t in threads:
        t.start()
    plugin.stop()
    for t in threads:
        t.join(10)
    assert ends == [grpc.StatusCode.OK] * 6
    assert not plugin._stream_subscriptions
    assert not os.path.exists(plugin.socket_path)
    # restart serves again and keeps counting
    before = plugin.allocations
    plugin.start(register=False)
    ch = grpc.insecure_channel(f"unix://{plugin.socket_path}")
    try:
        api.DevicePluginStub(ch).Allocate(_alloc_req(["70"]), timeout=5)
    finally:
        ch.close()
    assert plugin.allocations == before + 1


# ---------------------------------------------------------------------------
# concurrency and counters
# ---------------------------------------------------------------------------
def _rss_kb():
    with open("/proc/self/statm") as f:
        return int(f.read().split()[1]) * (os.sysconf("SC_PAGE_SIZE") // 1024)


def test_concurrent_admissions_counters_fds_rss(native):
    plugin = native.plugin()
    stubs = [native.stub() for _ in range(4)]
    errs = []

    def churn(ps, n):
        try:
            for i in range(n):
                gid = "70" if i % 2 else "71"
                resp = ps.Allocate(_alloc_req([gid]))
                assert resp.container_responses[0].cdi_devices[0].name.endswith(gid)
        except Exception as e:   # pragma: no cover
            errs.append(e)

    def run(n):
        threads = [threading.Thread(target=churn, args=(ps, n)) for ps in stubs]
        for t in threads:
            t.start()
        for t in threads:
            t.join()

    run(50)                       # warm allocators and channels
    base = plugin.allocations
    fds0 = len(os.listdir("/proc/self/fd"))
    rss = [_rss_kb()]
    for _ in range(5):
        run(100)
        rss.append(_rss_kb())
    assert not errs
    assert plugin.allocations - base == 2000
    assert plugin.allocate_failures == 0
    assert plugin.last_allocate_s > 0
    assert plugin.allocate_seconds_total >= plugin.last_allocate_s
    assert len(os.listdir("/proc/self/fd")) == fds0
    # not trending: the second half of the run may not keep growing. One
    # admission leaking even 1 KiB would add ~1.2 MiB over the last 1200.
    assert rss[-1] - rss[2] < 1024, rss
