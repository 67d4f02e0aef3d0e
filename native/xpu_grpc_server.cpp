// Native gRPC-over-HTTP/2 server for the device-plugin unix sockets.
//
// One GrpcServer owns one thread running a level-triggered epoll loop over
// its listening sockets and connections (protocol: h2.h / hpack.h). The
// loop runs without the GIL; it takes it only to call a registered Python
// unary (GetPreferredAllocation, the watcher-registration service) or to
// log a rejected Allocate.
//
//   Allocate                 fully native: table lookup, sysfs
//                            revalidation, response bytes concatenated
//                            from fragments prepared by update_table()
//   GetDevicePluginOptions,
//   PreStartContainer        constant response bytes
//   ListAndWatch             native streams fed by publish()
//
// Locking: table_mu_, pub_mu_ and stat_mu_ are leaf locks held for a few
// instructions. Python threads take them while holding the GIL (and the
// DeviceState lock); the loop thread never holds one while it waits for
// the GIL.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <fcntl.h>
#include <memory>
#include <mutex>
#include <poll.h>
#include <stdexcept>
#include <sys/epoll.h>
#include <sys/eventfd.h>
#include <sys/socket.h>
#include <sys/uio.h>
#include <sys/un.h>
#include <thread>
#include <unistd.h>
#include <unordered_map>

#include "h2.h"
#include "pbwire.h"

namespace py = pybind11;
using namespace kxdp;

namespace {

constexpr int STRATEGY_CDI_CRI = 0;
constexpr int STRATEGY_CDI_ANNOTATIONS = 1;
constexpr int STRATEGY_DEVICE_NODES = 2;
constexpr size_t kMaxTimingSamples = 1u << 20;

struct DeviceEntry {
    std::vector<std::string> bdfs;   // functions of the group, in order
    bool healthy = true;
    std::string cdi_device;          // serialised CDIDevice{name}
    std::string ann_key, ann_value;
    std::string dev_path;            // DeviceSpec host/container path
};

using Table = std::unordered_map<std::string, DeviceEntry>;

struct AllocateConfig {
    bool enabled = false;
    std::string path;
    int strategy = STRATEGY_CDI_CRI;
    bool reject_unhealthy = true;
    std::string cdi_kind, env_name, dev_root, devices_dir, required_driver;
    std::vector<long> vendors;
    bool timing = false;
};

enum class Kind { CONSTANT, WATCH, PYTHON, ALLOCATE };

struct Method {
    Kind kind;
    std::string bytes;     // CONSTANT
    py::object fn;         // PYTHON
};

std::string link_base(int dirfd, const char* name) {
    char buf[512];
    ssize_t n = ::readlinkat(dirfd, name, buf, sizeof(buf) - 1);
    if (n <= 0) return {};
    buf[n] = 0;
    const char* slash = std::strrchr(buf, '/');
    return std::string(slash ? slash + 1 : buf);
}

// sysfs `vendor` attribute as a number; -1 if unreadable
long read_vendor(int dirfd) {
    int fd = ::openat(dirfd, "vendor", O_RDONLY | O_CLOEXEC);
    if (fd < 0) return -1;
    char buf[64];
    ssize_t n = ::read(fd, buf, sizeof(buf) - 1);
    ::close(fd);
    if (n <= 0) return -1;
    buf[n] = 0;
    errno = 0;
    char* end = nullptr;
    long v = std::strtol(buf, &end, 16);
    if (errno || end == buf) return -1;
    return v;
}

struct IoConn {
    int fd;
    h2::Conn h2;
    size_t woff = 0;         // bytes of h2.out() already written
    size_t watching = 0;     // server streams already reported to Python
    bool want_write = false;
    IoConn(int f, h2::App* app) : fd(f), h2(app) {}
};

class GrpcServer : public h2::App {
public:
    explicit GrpcServer(std::vector<std::string> paths)
        : paths_(std::move(paths)) {}

    ~GrpcServer() override {
        if (thread_.joinable()) {
            py::gil_scoped_release rel;
            request_stop(0.0);
            thread_.join();
        }
        methods_.clear();
        on_reject_ = py::object();
        on_watch_change_ = py::object();
    }

    // ---- registration (before start) -----------------------------------
    void register_constant(const std::string& path, const std::string& bytes) {
        check_not_running();
        methods_[path] = Method{Kind::CONSTANT, bytes, py::object()};
    }
    // on_change(delta) is called from the loop (with the GIL) whenever
    // the number of open server streams changes — before the first message
    // of a new stream is written.
    void register_watch(const std::string& path, py::object on_change) {
        check_not_running();
        methods_[path] = Method{Kind::WATCH, {}, py::object()};
        on_watch_change_ = std::move(on_change);
    }
    void register_unary(const std::string& path, py::object fn) {
        check_not_running();
        methods_[path] = Method{Kind::PYTHON, {}, std::move(fn)};
    }
    void configure_allocate(const std::string& path, const std::string& strategy,
                            bool reject_unhealthy, const std::string& cdi_kind,
                            const std::string& env_name,
                            const std::string& dev_root,
                            const std::string& devices_dir,
                            const std::vector<long>& vendors,
                            const std::string& required_driver,
                            py::object on_reject, bool timing) {
        check_not_running();
        alloc_.enabled = true;
        alloc_.path = path;
        alloc_.strategy = strategy == "cdi-cri" ? STRATEGY_CDI_CRI
                          : strategy == "cdi-annotations" ? STRATEGY_CDI_ANNOTATIONS
                          : STRATEGY_DEVICE_NODES;
        alloc_.reject_unhealthy = reject_unhealthy;
        alloc_.cdi_kind = cdi_kind;
        alloc_.env_name = env_name;
        alloc_.dev_root = dev_root;
        alloc_.devices_dir = devices_dir;
        alloc_.vendors = vendors;
        alloc_.required_driver = required_driver;
        alloc_.timing = timing;
        on_reject_ = std::move(on_reject);
        methods_[path] = Method{Kind::ALLOCATE, {}, py::object()};
    }

    // ---- state pushed from Python (any thread, non-blocking) -----------
    // devices: (id, bdfs, healthy, cdi_device_bytes, ann_key, ann_value,
    // dev_path) per device
    void update_table(const std::vector<std::tuple<
            std::string, std::vector<std::string>, bool, py::bytes,
            std::string, std::string, std::string>>& devices) {
        auto t = std::make_shared<Table>();
        for (auto& d : devices) {
            DeviceEntry e;
            e.bdfs = std::get<1>(d);
            e.healthy = std::get<2>(d);
            e.cdi_device = std::string(std::get<3>(d));
            e.ann_key = std::get<4>(d);
            e.ann_value = std::get<5>(d);
            e.dev_path = std::get<6>(d);
            (*t)[std::get<0>(d)] = std::move(e);
        }
        std::lock_guard<std::mutex> g(table_mu_);
        table_ = std::move(t);
    }

    void publish(const std::string& message) {
        auto m = std::make_shared<const std::string>(message);
        {
            std::lock_guard<std::mutex> g(pub_mu_);
            latest_ = std::move(m);
            pub_gen_++;
        }
        wake();
    }

    // ---- lifecycle -------------------------------------------------------
    void start() {
        if (thread_.joinable()) throw std::runtime_error("server already started");
        stop_.store(false);
        ep_ = ::epoll_create1(EPOLL_CLOEXEC);
        wake_fd_ = ::eventfd(0, EFD_NONBLOCK | EFD_CLOEXEC);
        if (ep_ < 0 || wake_fd_ < 0) {
            close_fds();
            throw std::runtime_error("epoll/eventfd setup failed");
        }
        add_epoll(wake_fd_, EPOLLIN);
        for (auto& path : paths_) {
            sockaddr_un addr{};
            addr.sun_family = AF_UNIX;
            if (path.size() >= sizeof(addr.sun_path)) {
                close_fds();
                throw std::runtime_error("socket path too long: " + path);
            }
            std::memcpy(addr.sun_path, path.c_str(), path.size() + 1);
            int fd = ::socket(AF_UNIX, SOCK_STREAM | SOCK_NONBLOCK | SOCK_CLOEXEC, 0);
            if (fd < 0 || ::bind(fd, (sockaddr*)&addr, sizeof(addr)) < 0 ||
                ::listen(fd, 128) < 0) {
                std::string why = std::strerror(errno);
                if (fd >= 0) ::close(fd);
                close_fds();
                throw std::runtime_error("cannot listen on " + path + ": " + why);
            }
            listeners_.push_back(fd);
            bound_.push_back(path);
            add_epoll(fd, EPOLLIN);
        }
        thread_ = std::thread([this] { run(); });
    }

    // GOAWAY, end server streams with OK, flush for up to `grace` seconds,
    // close, unlink the sockets, join. Called with the GIL held: released
    // for the join because the loop may be waiting for it.
    void stop(double grace) {
        if (!thread_.joinable()) return;
        py::gil_scoped_release rel;
        request_stop(grace);
        thread_.join();
    }

    bool running() const { return thread_.joinable(); }

    py::tuple stats() {
        std::lock_guard<std::mutex> g(stat_mu_);
        return py::make_tuple(allocations_, failures_, last_s_, total_s_);
    }

    std::vector<double> allocate_timing_us() {
        std::lock_guard<std::mutex> g(stat_mu_);
        return alloc_us_;
    }

    // ---- h2::App -----------------------------------------------------------
    void on_rpc(h2::Conn& c, uint32_t sid, const std::string& path,
                std::string& msg) override {
        auto it = methods_.find(path);
        if (it == methods_.end())
            return c.reply_error(sid, h2::GRPC_UNIMPLEMENTED, "Method not found!");
        Method& m = it->second;
        switch (m.kind) {
        case Kind::CONSTANT:
            return c.reply_unary(sid, m.bytes);
        case Kind::ALLOCATE:
            return handle_allocate(c, sid, msg);
        case Kind::WATCH: {
            std::shared_ptr<const std::string> latest;
            {
                std::lock_guard<std::mutex> g(pub_mu_);
                latest = latest_;
            }
            c.start_stream(sid);
            if (latest) c.push_message(sid, *latest);
            return;
        }
        case Kind::PYTHON:
            return handle_python(c, sid, m, msg);
        }
    }

private:
    void check_not_running() {
        if (thread_.joinable())
            throw std::runtime_error("register methods before start()");
    }

    void wake() {
        if (wake_fd_ >= 0) {
            uint64_t one = 1;
            ssize_t r = ::write(wake_fd_, &one, sizeof(one));
            (void)r;
        }
    }

    void request_stop(double grace) {
        grace_s_ = grace;
        stop_.store(true);
        wake();
    }

    void add_epoll(int fd, uint32_t events) {
        epoll_event ev{};
        ev.events = events;
        ev.data.fd = fd;
        ::epoll_ctl(ep_, EPOLL_CTL_ADD, fd, &ev);
    }

    void close_fds() {
        for (int fd : listeners_) ::close(fd);
        listeners_.clear();
        for (auto& p : bound_) ::unlink(p.c_str());
        bound_.clear();
        if (wake_fd_ >= 0) ::close(wake_fd_);
        if (ep_ >= 0) ::close(ep_);
        wake_fd_ = ep_ = -1;
        if (dirfd_ >= 0) ::close(dirfd_);
        dirfd_ = -1;
        dirfd_table_ = nullptr;
    }

    // ---- Python calls from the loop thread --------------------------------
    // The loop thread keeps ONE thread state for its lifetime and swaps it
    // in and out around each call.
    struct GilHold {
        PyThreadState*& ts;
        bool held = false;
        explicit GilHold(PyThreadState*& t) : ts(t) {
            if (ts && !_Py_IsFinalizing()) {
                PyEval_RestoreThread(ts);
                held = true;
            }
        }
        ~GilHold() {
            if (held) ts = PyEval_SaveThread();
        }
    };

    void handle_python(h2::Conn& c, uint32_t sid, Method& m, std::string& msg) {
        bool ok = false;
        int status = h2::GRPC_UNKNOWN;
        std::string payload;
        {
            GilHold gil(ts_);
            if (!gil.held) {
                status = h2::GRPC_UNAVAILABLE;
                payload = "server shutting down";
            } else {
                try {
                    py::object r = m.fn(py::bytes(msg));
                    if (py::isinstance<py::bytes>(r)) {
                        payload = r.cast<std::string>();
                        ok = true;
                    } else {   // (status code, message)
                        auto t = r.cast<std::pair<int, std::string>>();
                        status = t.first;
                        payload = t.second;
                    }
                } catch (py::error_already_set& e) {
                    try {
                        payload = "Unexpected " +
                                  py::str(e.type()).cast<std::string>() + ": " +
                                  py::str(e.value()).cast<std::string>();
                    } catch (...) {
                        payload = "handler raised";
                    }
                    e.restore();
                    PyErr_Clear();
                } catch (std::exception& e) {
                    payload = e.what();
                }
            }
        }
        if (ok) c.reply_unary(sid, payload);
        else c.reply_error(sid, status, payload);
    }

    void report_watchers(IoConn& io, size_t now) {
        if (now == io.watching) return;
        long delta = (long)now - (long)io.watching;
        io.watching = now;
        GilHold gil(ts_);
        if (!gil.held || !on_watch_change_ || on_watch_change_.is_none()) return;
        try {
            on_watch_change_(delta);
        } catch (py::error_already_set& e) {
            e.restore();
            PyErr_Clear();
        }
    }

    void log_rejection(const std::string& err) {
        GilHold gil(ts_);
        if (!gil.held || !on_reject_ || on_reject_.is_none()) return;
        try {
            on_reject_(err);
        } catch (py::error_already_set& e) {
            e.restore();
            PyErr_Clear();
        }
    }

    // ---- Allocate ------------------------------------------------------------
    bool open_devices_dir() {
        if (dirfd_ >= 0) ::close(dirfd_);
        dirfd_ = ::open(alloc_.devices_dir.c_str(),
                        O_RDONLY | O_DIRECTORY | O_CLOEXEC);
        return dirfd_ >= 0;
    }

    // Same checks and messages as revalidate_groups() in xpu_native.cpp, but
    // the devices-dir fd stays open across calls.
    std::string revalidate(const std::string& gid, const DeviceEntry& dev) {
        for (const auto& bdf : dev.bdfs) {
            const int flags = O_RDONLY | O_DIRECTORY | O_CLOEXEC;
            int dfd = ::openat(dirfd_, bdf.c_str(), flags);
            if (dfd < 0) {   // the directory itself may have been replaced
                if (!open_devices_dir())
                    return "cannot open " + alloc_.devices_dir;
                dfd = ::openat(dirfd_, bdf.c_str(), flags);
            }
            if (dfd < 0) return "device " + bdf + " vanished";
            std::string err;
            if (link_base(dfd, "iommu_group") != gid) {
                err = "device " + bdf + " no longer in IOMMU group " + gid;
            } else {
                long vendor = read_vendor(dfd);
                if (vendor < 0 ||
                    std::find(alloc_.vendors.begin(), alloc_.vendors.end(),
                              vendor) == alloc_.vendors.end())
                    err = "device " + bdf + " vendor not allowed";
                else if (link_base(dfd, "driver") != alloc_.required_driver)
                    err = "device " + bdf + " not bound to " +
                          alloc_.required_driver;
            }
            ::close(dfd);
            if (!err.empty()) return err;
        }
        return {};
    }

    std::string allocate_container(const Table& table,
                                   const std::vector<std::string>& ids,
                                   std::string& out) {
        std::vector<const DeviceEntry*> devs;
        devs.reserve(ids.size());
        for (const auto& gid : ids) {
            auto it = table.find(gid);
            if (it == table.end()) return "unknown device id " + gid;
            if (alloc_.reject_unhealthy && !it->second.healthy)
                return "device " + gid + " is Unhealthy";
            devs.push_back(&it->second);
        }
        if (dirfd_ < 0 || dirfd_table_ != &table) {
            if (!open_devices_dir()) return "cannot open " + alloc_.devices_dir;
            dirfd_table_ = &table;
        }
        for (size_t i = 0; i < ids.size(); i++) {
            std::string err = revalidate(ids[i], *devs[i]);
            if (!err.empty()) return err;
        }
        const bool cdi = alloc_.strategy != STRATEGY_DEVICE_NODES;
        std::string bdfs;
        for (auto* d : devs)
            for (const auto& b : d->bdfs) {
                if (!bdfs.empty()) bdfs.push_back(',');
                bdfs += b;
            }
        // envs (field 1), in key order like a deterministic serialiser
        static const std::string kVendorClass = "KUBERNETES_CDI_VENDOR_CLASS";
        if (cdi && alloc_.env_name == kVendorClass) {
            pb::put_map_entry(out, 1, alloc_.env_name, bdfs);   // later set wins
        } else if (cdi && kVendorClass < alloc_.env_name) {
            pb::put_map_entry(out, 1, kVendorClass, alloc_.cdi_kind);
            pb::put_map_entry(out, 1, alloc_.env_name, bdfs);
        } else {
            pb::put_map_entry(out, 1, alloc_.env_name, bdfs);
            if (cdi) pb::put_map_entry(out, 1, kVendorClass, alloc_.cdi_kind);
        }
        if (!cdi) {   // devices (field 3)
            auto spec = [&](const std::string& path) {
                std::string s;
                pb::put_bytes(s, 1, path);
                pb::put_bytes(s, 2, path);
                pb::put_bytes(s, 3, "rw", 2);
                pb::put_bytes(out, 3, s);
            };
            if (!ids.empty()) spec(alloc_.dev_root + "/vfio/vfio");
            for (auto* d : devs) spec(d->dev_path);
        }
        if (alloc_.strategy == STRATEGY_CDI_ANNOTATIONS)
            for (auto* d : devs)
                pb::put_map_entry(out, 4, d->ann_key, d->ann_value);
        if (alloc_.strategy == STRATEGY_CDI_CRI)
            for (auto* d : devs) pb::put_bytes(out, 5, d->cdi_device);
        return {};
    }

    void handle_allocate(h2::Conn& c, uint32_t sid, const std::string& msg) {
        auto t0 = std::chrono::steady_clock::now();
        std::shared_ptr<const Table> table;
        {
            std::lock_guard<std::mutex> g(table_mu_);
            table = table_;
        }
        std::vector<std::vector<std::string>> reqs;
        if (!pb::parse_allocate_request(msg, reqs))
            return c.reply_error(sid, h2::GRPC_INTERNAL,
                                 "Exception deserializing request!");
        static const Table kEmpty;
        const Table& tbl = table ? *table : kEmpty;
        std::string resp, err;
        for (const auto& ids : reqs) {
            std::string cresp;
            err = allocate_container(tbl, ids, cresp);
            if (!err.empty()) break;
            pb::put_bytes(resp, 1, cresp);
        }
        if (!err.empty()) {
            {
                std::lock_guard<std::mutex> g(stat_mu_);
                failures_++;
            }
            c.reply_error(sid, h2::GRPC_INVALID_ARGUMENT, err);
            log_rejection(err);
            return;
        }
        double dt = std::chrono::duration<double>(
                        std::chrono::steady_clock::now() - t0).count();
        {
            std::lock_guard<std::mutex> g(stat_mu_);
            allocations_++;
            last_s_ = dt;
            total_s_ += dt;
            if (alloc_.timing && alloc_us_.size() < kMaxTimingSamples)
                alloc_us_.push_back(dt * 1e6);
        }
        c.reply_unary(sid, resp);
    }

    // ---- IO loop ------------------------------------------------------------------
    void set_want_write(IoConn& io, bool on) {
        if (io.want_write == on) return;
        io.want_write = on;
        epoll_event ev{};
        ev.events = EPOLLIN | (on ? EPOLLOUT : 0);
        ev.data.fd = io.fd;
        ::epoll_ctl(ep_, EPOLL_CTL_MOD, io.fd, &ev);
    }

    // Write what h2 queued — one gathered write per batch of replies.
    // Returns false if the connection is finished (caller closes it).
    bool flush(IoConn& io) {
        std::string& out = io.h2.out();
        while (io.woff < out.size()) {
            iovec iov{(void*)(out.data() + io.woff), out.size() - io.woff};
            msghdr mh{};
            mh.msg_iov = &iov;
            mh.msg_iovlen = 1;
            ssize_t n = ::sendmsg(io.fd, &mh, MSG_NOSIGNAL);
            if (n < 0) {
                if (errno == EINTR) continue;
                if (errno == EAGAIN || errno == EWOULDBLOCK) {
                    set_want_write(io, true);
                    return true;
                }
                return false;
            }
            io.woff += (size_t)n;
        }
        out.clear();
        io.woff = 0;
        set_want_write(io, false);
        return !io.h2.want_close();
    }

    void close_conn(int fd) {
        auto it = conns_.find(fd);
        if (it == conns_.end()) return;
        report_watchers(*it->second, 0);
        ::epoll_ctl(ep_, EPOLL_CTL_DEL, fd, nullptr);
        ::close(fd);
        conns_.erase(it);
    }

    void on_readable(IoConn& io) {
        ssize_t n = ::read(io.fd, rbuf_, sizeof(rbuf_));
        if (n == 0) return close_conn(io.fd);          // peer closed
        if (n < 0) {
            if (errno == EAGAIN || errno == EINTR) return;
            return close_conn(io.fd);
        }
        io.h2.feed((const uint8_t*)rbuf_, (size_t)n);
        report_watchers(io, io.h2.watch_streams());
        if (!flush(io)) close_conn(io.fd);
    }

    void deliver_publications() {
        std::shared_ptr<const std::string> latest;
        uint64_t gen;
        {
            std::lock_guard<std::mutex> g(pub_mu_);
            latest = latest_;
            gen = pub_gen_;
        }
        if (gen == pub_seen_ || !latest) return;
        pub_seen_ = gen;
        std::vector<int> done;
        for (auto& kv : conns_) {
            kv.second->h2.broadcast(*latest);
            if (!flush(*kv.second)) done.push_back(kv.first);
        }
        for (int fd : done) close_conn(fd);
    }

    void shutdown_connections() {
        for (int fd : listeners_) ::close(fd);
        listeners_.clear();
        for (auto& p : bound_) ::unlink(p.c_str());
        bound_.clear();
        for (auto& kv : conns_) kv.second->h2.begin_shutdown();
        auto deadline = std::chrono::steady_clock::now() +
                        std::chrono::duration<double>(grace_s_);
        for (auto& kv : conns_) {
            IoConn& io = *kv.second;
            while (flush(io) && io.woff < io.h2.out().size()) {
                auto left = std::chrono::duration_cast<std::chrono::milliseconds>(
                    deadline - std::chrono::steady_clock::now()).count();
                if (left <= 0) break;
                pollfd p{io.fd, POLLOUT, 0};
                if (::poll(&p, 1, (int)left) <= 0) break;
            }
            // Half-close and drop what the peer already sent, so close()
            // finds no unread data and the peer reads our last frames.
            ::shutdown(io.fd, SHUT_WR);
            while (::read(io.fd, rbuf_, sizeof(rbuf_)) > 0) {}
            report_watchers(io, 0);
            ::close(io.fd);
        }
        conns_.clear();
    }

    void run() {
        PyGILState_STATE gstate = PyGILState_Ensure();
        ts_ = PyEval_SaveThread();
        epoll_event evs[64];
        while (!stop_.load()) {
            int n = ::epoll_wait(ep_, evs, 64, -1);
            if (n < 0) {
                if (errno == EINTR) continue;
                break;
            }
            for (int i = 0; i < n && !stop_.load(); i++) {
                int fd = evs[i].data.fd;
                if (fd == wake_fd_) {
                    uint64_t v;
                    while (::read(wake_fd_, &v, sizeof(v)) > 0) {}
                    deliver_publications();
                    continue;
                }
                if (std::find(listeners_.begin(), listeners_.end(), fd) !=
                    listeners_.end()) {
                    for (;;) {
                        int cfd = ::accept4(fd, nullptr, nullptr,
                                            SOCK_NONBLOCK | SOCK_CLOEXEC);
                        if (cfd < 0) break;
                        auto io = std::make_unique<IoConn>(cfd, this);
                        IoConn& ref = *io;
                        conns_[cfd] = std::move(io);
                        add_epoll(cfd, EPOLLIN);
                        if (!flush(ref)) close_conn(cfd);   // our SETTINGS
                    }
                    continue;
                }
                auto it = conns_.find(fd);
                if (it == conns_.end()) continue;   // closed earlier this round
                IoConn& io = *it->second;
                if (evs[i].events & EPOLLOUT) {
                    if (!flush(io)) {
                        close_conn(fd);
                        continue;
                    }
                }
                if (evs[i].events & (EPOLLIN | EPOLLHUP | EPOLLERR))
                    on_readable(io);   // EOF / error surfaces from read()
            }
        }
        shutdown_connections();
        if (!_Py_IsFinalizing()) {
            PyEval_RestoreThread(ts_);
            PyGILState_Release(gstate);
        }
        ts_ = nullptr;
        int ep = ep_, wfd = wake_fd_;
        ep_ = wake_fd_ = -1;
        ::close(ep);
        ::close(wfd);
        if (dirfd_ >= 0) ::close(dirfd_);
        dirfd_ = -1;
        dirfd_table_ = nullptr;
    }

    std::vector<std::string> paths_, bound_;
    std::unordered_map<std::string, Method> methods_;
    AllocateConfig alloc_;
    py::object on_reject_, on_watch_change_;

    std::mutex table_mu_;
    std::shared_ptr<const Table> table_;
    std::mutex pub_mu_;
    std::shared_ptr<const std::string> latest_;
    uint64_t pub_gen_ = 0;
    uint64_t pub_seen_ = 0;      // loop thread only

    std::mutex stat_mu_;
    uint64_t allocations_ = 0, failures_ = 0;
    double last_s_ = 0.0, total_s_ = 0.0;
    std::vector<double> alloc_us_;

    std::thread thread_;
    std::atomic<bool> stop_{false};
    double grace_s_ = 1.0;
    int ep_ = -1, wake_fd_ = -1;
    std::vector<int> listeners_;
    std::unordered_map<int, std::unique_ptr<IoConn>> conns_;   // loop thread
    PyThreadState* ts_ = nullptr;                               // loop thread
    int dirfd_ = -1;                                            // loop thread
    const Table* dirfd_table_ = nullptr;
    char rbuf_[65536];
};

}  // namespace

void kxdp_init_grpc_server(py::module_& m) {
    py::class_<GrpcServer>(m, "GrpcServer")
        .def(py::init<std::vector<std::string>>(), py::arg("socket_paths"))
        .def("register_constant", &GrpcServer::register_constant,
             py::arg("path"), py::arg("response"))
        .def("register_watch", &GrpcServer::register_watch, py::arg("path"),
             py::arg("on_change") = py::none())
        .def("register_unary", &GrpcServer::register_unary, py::arg("path"),
             py::arg("fn"),
             "fn(request bytes) -> response bytes | (status code, message)")
        .def("configure_allocate", &GrpcServer::configure_allocate,
             py::arg("path"), py::arg("strategy"), py::arg("reject_unhealthy"),
             py::arg("cdi_kind"), py::arg("env_name"), py::arg("dev_root"),
             py::arg("devices_dir"), py::arg("vendors"),
             py::arg("required_driver"), py::arg("on_reject"),
             py::arg("timing") = false)
        .def("update_table", &GrpcServer::update_table, py::arg("devices"))
        .def("publish", &GrpcServer::publish, py::arg("message"))
        .def("start", &GrpcServer::start)
        .def("stop", &GrpcServer::stop, py::arg("grace") = 1.0)
        .def("stats", &GrpcServer::stats)
        .def("allocate_timing_us", &GrpcServer::allocate_timing_us)
        .def_property_readonly("running", &GrpcServer::running);
}
