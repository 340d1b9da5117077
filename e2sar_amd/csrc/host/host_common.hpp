// host_common.hpp -- internal helpers shared by the Segmenter/Reassembler façade.
#pragma once

#include <netinet/in.h>
#include <sys/socket.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <map>
#include <memory>
#include <string>
#include <utility>

#include "e2sar_amd/e2sar.hpp"
#include "e2sar_hip.h"

namespace e2sar {
namespace detail {

bool read_ini(const std::string &path, std::map<std::string, std::string> &out, std::string &err);
bool ini_bool(const std::map<std::string, std::string> &m, const std::string &k, bool def);
double ini_num(const std::map<std::string, std::string> &m, const std::string &k, double def);

// C-ABI status -> E2SARErrorInfo (status = -(E2SARErrorc))
inline E2SARErrorInfo hip_error(int rc, const std::string &what)
{
    return E2SARErrorInfo{static_cast<E2SARErrorc>(-rc), what + ": " + e2sar_hip_last_error()};
}

inline uint64_t now_us()
{
    return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
               std::chrono::system_clock::now().time_since_epoch())
        .count();
}

// clockEntropyTest (e2sarUtil.hpp:549-574): Shannon entropy, in bits, of the low 8 bits of
// the microsecond wall clock sampled every sleepMs; measured once per process (the clock
// does not change under it) -- the reference measures it in every Segmenter constructor
float clock_entropy_bits();

// Segmenter MTU rules (segmenter.cpp): interface/override resolution and the 9000-byte limit
uint32_t resolve_mtu(uint16_t flagsMtu, uint32_t ifMtu, const std::string &iface);
void check_mtu_limit(uint32_t mtu);
EventNum_t take_send_number(std::atomic<EventNum_t> &userEventNum, EventNum_t eventNum, size_t depth, size_t cap,
                            bool *accepted);

inline uint64_t steady_ms()
{
    return (uint64_t)std::chrono::duration_cast<std::chrono::milliseconds>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

// ---- move-only owners of what the C ABI hands out ----
template <auto Destroy> struct Deleter {
    template <class T> void operator()(T *p) const { Destroy(p); }
};
struct DeviceFree {
    e2sar_hip_ctx *ctx = nullptr;      // e2sar_hip_device_free needs it: the buffer goes before its context
    void operator()(void *p) const { e2sar_hip_device_free(ctx, p); }
};
template <class T> using Pinned = std::unique_ptr<T[], Deleter<e2sar_hip_host_free>>;
template <class T> using DeviceBuf = std::unique_ptr<T[], DeviceFree>;
using Stream = std::unique_ptr<void, Deleter<e2sar_hip_stream_destroy>>;
using Event = std::unique_ptr<void, Deleter<e2sar_hip_event_destroy>>;
using Ctx = std::unique_ptr<e2sar_hip_ctx, Deleter<e2sar_hip_ctx_destroy>>;
using Reas = std::unique_ptr<e2sar_hip_reas, Deleter<e2sar_hip_reas_destroy>>;

// rc = create(args..., &handle), the handle into its owner
template <class Owner, class Create, class... Args> int make(Owner &out, Create create, Args... args)
{
    typename Owner::pointer p = nullptr;
    const int rc = create(args..., &p);
    out.reset(p);
    return rc;
}
// `count` elements into `out`, whose old buffer is released first (the caller has synchronised
// the stream it was used on); a failure leaves `out` empty
template <class T> int alloc_pinned(size_t count, Pinned<T> &out)
{
    out.reset();
    void *p = nullptr;
    const int rc = e2sar_hip_host_alloc(count * sizeof(T), &p);
    out.reset(static_cast<T *>(p));
    return rc;
}
template <class T> int alloc_device(e2sar_hip_ctx *ctx, size_t count, DeviceBuf<T> &out)
{
    out.reset();
    void *p = nullptr;
    const int rc = e2sar_hip_device_alloc(ctx, count * sizeof(T), &p);
    out = DeviceBuf<T>(static_cast<T *>(p), DeviceFree{ctx});
    return rc;
}

// a file descriptor, closed once
class Fd {
    int fd_ = -1;
public:
    explicit Fd(int fd = -1) : fd_(fd) {}
    Fd(Fd &&o) noexcept : fd_(o.fd_) { o.fd_ = -1; }
    Fd &operator=(Fd &&o) noexcept { return std::swap(fd_, o.fd_), *this; }
    ~Fd() { reset(); }
    int get() const { return fd_; }
    bool valid() const { return fd_ >= 0; }
    void reset(int fd = -1)
    {
        if (fd_ >= 0) ::close(fd_);
        fd_ = fd;
    }
};

// The one sockaddr_in / sockaddr_in6 fill (util.cpp): `host` as text of the family (empty =
// its wildcard address) and `port`; ok is false for text inet_pton rejects for that family
struct SockAddr {
    sockaddr_storage ss{};
    socklen_t len = 0;
    bool ok = false;
    const sockaddr *sa() const { return reinterpret_cast<const sockaddr *>(&ss); }
};
SockAddr sock_addr(const std::string &host, uint16_t port, bool v6);

}  // namespace detail
}  // namespace e2sar
