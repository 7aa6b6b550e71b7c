// HBM seeding: a BEP XET server whose piece provider reads serialized xorbs resident in GPU
// memory (BASELINE config "Mixtral-8x7B seed mode: serve xorbs from 288 GB HBM").
//
// Each request [range_start, range_end) of a registered xorb is copied HBM -> a per-connection
// pinned staging buffer (hipMemcpyAsync on a per-thread stream) and written to the socket straight
// from that buffer (zero-copy CacheHit), so a served byte crosses PCIe once and is never copied on
// the host.  Xorbs not in HBM fall through to the disk cache like `zest serve`.
//
// Resident runs serve the same requests from decoded bytes that are already in HBM as tensors (a
// device pull's file buffers): instead of a copy, each piece is serialised by zg_serve_pack
// (gpu/serve.hip) straight into the pinned staging buffer, from two small device tables per run
// (chunk addresses + serialized ends, 16 B per chunk) -- no serialized second copy of the model.
// Every chunk of a resident run must lie inside a buffer registered with add_resident_buffer, and
// the device tables are read back and checked at registration, so the kernel never runs on an
// address nobody vouched for.
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cstdlib>
#include <memory>
#include <shared_mutex>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../gpu/zgpu.h"
#include "bt_server.h"
#include "config.h"
#include "storage.h"
#include "xet_hash.h"

namespace py = pybind11;
using namespace zest;

namespace {

struct XorbLoc {
  uint64_t dev_off;                 // serialized run start inside the device arena
  std::vector<uint64_t> ends;       // serialized end offset of each chunk (relative to dev_off)
  uint32_t first = 0;               // xorb chunk index of the run's first chunk (partial runs)
  // resident run (src_tab != null): device tables of chunk addresses / serialized ends; dev_off unused
  const uint64_t* src_tab = nullptr;
  const uint64_t* end_tab = nullptr;
};

// Per connection thread: pinned staging for one response, the stream its D2H copies run on, and one
// event per piece.  A thread serves one request at a time, so the next response reuses them only after
// the previous one was sent.
struct Staging {
  uint8_t* host = nullptr;
  uint8_t* host_dev = nullptr;  // the address kernels write `host` at (resident runs)
  size_t cap = 0;
  hipStream_t stream = nullptr;
  std::vector<hipEvent_t> ev;
  ~Staging() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    if (host) (void)hipHostFree(host);
    if (stream) (void)hipStreamDestroy(stream);
  }
  void ensure(size_t n, size_t pieces) {
    while (ev.size() < pieces) {
      hipEvent_t e = nullptr;
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) throw Error("HipError", "hipEventCreate");
      ev.push_back(e);
    }
    if (n <= cap) return;
    if (host) (void)hipHostFree(host);
    host = nullptr;
    cap = 0;
    if (hipHostMalloc(reinterpret_cast<void**>(&host), n, hipHostMallocDefault) != hipSuccess)
      throw Error("HipError", "hipHostMalloc staging");
    if (hipHostGetDevicePointer(reinterpret_cast<void**>(&host_dev), host, 0) != hipSuccess)
      throw Error("HipError", "staging buffer is not device-visible");
    cap = n;
  }
};

class HbmSeeder {
 public:
  HbmSeeder(uintptr_t arena, uint64_t arena_bytes, int device, int port, bool disk_fallback)
      : arena_(reinterpret_cast<const uint8_t*>(arena)), arena_n_(arena_bytes), device_(device),
        cfg_(Config::from_env()) {
    if (disk_fallback) {
      registry_.scan(cfg_);
      cache_ = std::make_unique<storage::XorbCache>(cfg_, &registry_);
    }
    server_ = std::make_unique<bt::BtServer>(
        cfg_, cache_.get(),
        [this](const std::array<uint8_t, 32>&, const std::string& hex, uint32_t a, uint32_t b) {
          return provide(hex, a, b);
        },
        port);
  }
  ~HbmSeeder() { stop(); }

  void add_xorb(const std::string& hex, uint64_t dev_off, std::vector<uint64_t> ends, uint32_t first) {
    if (ends.empty() || dev_off + ends.back() > arena_n_) throw Error("InvalidRange", "xorb outside arena");
    std::unique_lock<std::shared_mutex> g(mu_);
    index_[hex].push_back(XorbLoc{dev_off, std::move(ends), first});  // several runs per xorb allowed
  }

  // A device range that resident runs may read (a pulled file's buffer): must lie inside one
  // device allocation.
  void add_resident_buffer(uintptr_t ptr, uint64_t nbytes) {
    (void)hipSetDevice(device_);
    if (!in_one_allocation(ptr, nbytes)) throw Error("InvalidRange", "resident buffer is not inside a device allocation");
    std::unique_lock<std::shared_mutex> g(mu_);
    buffers_.emplace_back(ptr, ptr + nbytes);
  }

  // Chunks [first, first + n) of xorb `hex`, served by zg_serve_pack from the device tables
  // src_tab[n] (chunk addresses) and end_tab[n] (== ends, the serialized end offsets).  The tables
  // are copied back once and checked: ends must match, every length must fit a u24 header and every
  // chunk must lie inside a registered buffer.
  void add_resident_run(const std::string& hex, uint32_t first, uintptr_t src_tab, uintptr_t end_tab,
                        std::vector<uint64_t> ends) {
    const size_t n = ends.size();
    if (n == 0 || n > 0xFFFFFFFFull - first) throw Error("InvalidRange", "empty resident run");
    if (!src_tab || !end_tab || (src_tab & 7) || (end_tab & 7)) throw Error("InvalidRange", "resident run tables");
    (void)hipSetDevice(device_);
    std::vector<uint64_t> src(n), dev_ends(n);
    if (!in_one_allocation(src_tab, 8 * n) || !in_one_allocation(end_tab, 8 * n) ||
        hipMemcpy(src.data(), reinterpret_cast<const void*>(src_tab), 8 * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(dev_ends.data(), reinterpret_cast<const void*>(end_tab), 8 * n, hipMemcpyDeviceToHost) != hipSuccess) {
      (void)hipGetLastError();
      throw Error("InvalidRange", "resident run tables are not readable device memory");
    }
    if (dev_ends != ends) throw Error("InvalidRange", "resident run: device ser_end table differs from chunk_ends");
    std::unique_lock<std::shared_mutex> g(mu_);
    uint64_t prev = 0;
    for (size_t i = 0; i < n; ++i) {
      if (ends[i] < prev + 8) throw Error("InvalidRange", "resident run: chunk ends not increasing");
      const uint64_t len = ends[i] - prev - 8;
      prev = ends[i];
      if (len >= (uint64_t(1) << 24)) throw Error("InvalidRange", "resident run: chunk too large for a u24 header");
      if (len == 0) continue;
      bool ok = false;
      for (const auto& b : buffers_)
        if (src[i] >= b.first && src[i] + len >= src[i] && src[i] + len <= b.second) {
          ok = true;
          break;
        }
      if (!ok) throw Error("InvalidRange", "resident run: chunk outside every registered buffer");
    }
    XorbLoc x{0, std::move(ends), first};
    x.src_tab = reinterpret_cast<const uint64_t*>(src_tab);
    x.end_tab = reinterpret_cast<const uint64_t*>(end_tab);
    index_[hex].push_back(std::move(x));
    ++resident_runs_;
  }
  size_t resident_runs() const {
    std::shared_lock<std::shared_mutex> g(mu_);
    return resident_runs_;
  }
  size_t count() const {
    std::shared_lock<std::shared_mutex> g(mu_);
    return index_.size();
  }
  void start() { server_->start(); }
  void stop() {
    if (server_) server_->stop();
  }
  uint16_t port() const { return server_->port(); }
  bt::ServerStats stats() const { return server_->stats(); }

 private:
  // [ptr, ptr + nbytes) lies inside one allocation the HIP runtime knows.
  static bool in_one_allocation(uintptr_t ptr, uint64_t nbytes) {
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (!ptr || !nbytes || ptr + nbytes < ptr ||
        hipMemGetAddressRange(&base, &size, reinterpret_cast<hipDeviceptr_t>(ptr)) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(base);
    return ptr >= b0 && ptr + nbytes <= b0 + size;
  }

  std::optional<storage::CacheHit> provide(const std::string& hex, uint32_t a, uint32_t b) {
    uint64_t lo, hi;
    const uint64_t *src_tab = nullptr, *end_tab = nullptr;
    uint32_t run_n = 0;
    {
      std::shared_lock<std::shared_mutex> g(mu_);
      auto it = index_.find(hex);
      if (it == index_.end()) return std::nullopt;
      const XorbLoc* hit = nullptr;
      uint32_t bb = b;
      for (const XorbLoc& x : it->second) {  // first run covering [a, b)
        const uint32_t n = x.first + uint32_t(x.ends.size());
        const uint32_t want_end = b == 0 ? n : b;
        if (a >= x.first && a < want_end && want_end <= n) {
          hit = &x;
          bb = want_end;
          break;
        }
      }
      if (!hit) return std::nullopt;
      const uint32_t ra = a - hit->first, rb = bb - hit->first;
      lo = hit->dev_off + (ra ? hit->ends[ra - 1] : 0);
      hi = hit->dev_off + hit->ends[rb - 1];
      src_tab = hit->src_tab;  // resident run: lo / hi are offsets in the run's serialized stream
      end_tab = hit->end_tab;
      run_n = uint32_t(hit->ends.size());
    }
    thread_local std::shared_ptr<Staging> st;
    if (!st) {
      st = std::make_shared<Staging>();
      (void)hipSetDevice(device_);
      if (hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking) != hipSuccess)
        throw Error("HipError", "hipStreamCreate");
    }
    // The response is copied HBM -> pinned in pieces of kPiece (ZEST_SEED_PIECE_MB, default 8)
    // queued back to back, each followed by an event: the server sends piece k while piece k + 1 is
    // still in flight (ready() waits for the piece a slice needs), instead of copying the whole
    // run (up to 64 MiB) and synchronizing before the first byte goes out.
    static const size_t kPiece = [] {
      const char* v = std::getenv("ZEST_SEED_PIECE_MB");
      const size_t mb = v && *v ? size_t(std::strtoull(v, nullptr, 10)) : 8;
      return std::max<size_t>(1, mb) << 20;
    }();
    const size_t len = size_t(hi - lo);
    const size_t pieces = std::max<size_t>(1, (len + kPiece - 1) / kPiece);
    st->ensure(len, pieces);
    for (size_t k = 0; k < pieces; ++k) {
      const size_t o = k * kPiece, n = std::min(kPiece, len - o);
      // serialized run: copy; resident run: serialise the piece into the staging buffer (pinned host
      // memory the GPU writes directly; o is a multiple of the piece size, so it stays 16-byte aligned)
      const hipError_t e =
          !n ? hipSuccess
             : src_tab ? zg_serve_pack(src_tab, end_tab, run_n, lo + o, lo + o + n, st->host_dev + o, st->stream)
                       : hipMemcpyAsync(st->host + o, arena_ + lo + o, n, hipMemcpyDeviceToHost, st->stream);
      if (e != hipSuccess || hipEventRecord(st->ev[k], st->stream) != hipSuccess)
        throw Error("HipError", "HBM -> host copy");
    }
    storage::CacheHit h;
    h.chunk_offset = a;
    h.ext = st->host;
    h.ext_len = len;
    h.keep = st;
    Staging* sp = st.get();
    h.ready = [sp](size_t upto) {
      if (!upto) return;
      const size_t k = (upto - 1) / kPiece;
      if (hipEventSynchronize(sp->ev[std::min(k, sp->ev.size() - 1)]) != hipSuccess)
        throw Error("HipError", "HBM -> host copy");
    };
    return h;
  }

  const uint8_t* arena_;
  uint64_t arena_n_;
  int device_;
  Config cfg_;
  storage::XorbRegistry registry_;
  std::unique_ptr<storage::XorbCache> cache_;
  std::unique_ptr<bt::BtServer> server_;
  mutable std::shared_mutex mu_;
  std::unordered_map<std::string, std::vector<XorbLoc>> index_;
  std::vector<std::pair<uintptr_t, uintptr_t>> buffers_;  // [begin, end) device ranges resident runs may read
  size_t resident_runs_ = 0;
};

}  // namespace

void bind_hip_seed(py::module_& m) {
  py::class_<HbmSeeder>(m, "HbmSeeder", "BEP XET seeder serving serialized xorbs from HBM")
      .def(py::init<uintptr_t, uint64_t, int, int, bool>(), py::arg("arena_ptr"), py::arg("arena_bytes"),
           py::arg("device") = 0, py::arg("port") = 0, py::arg("disk_fallback") = false)
      .def("add_xorb", &HbmSeeder::add_xorb, py::arg("xet_hex"), py::arg("dev_off"), py::arg("chunk_ends"),
           py::arg("first_chunk") = 0)
      .def("add_resident_buffer", &HbmSeeder::add_resident_buffer, py::arg("ptr"), py::arg("nbytes"),
           "register a device range that resident runs may read")
      .def("add_resident_run", &HbmSeeder::add_resident_run, py::arg("xet_hex"), py::arg("first_chunk"),
           py::arg("src_table_ptr"), py::arg("ser_end_table_ptr"), py::arg("chunk_ends"),
           "chunks [first_chunk, first_chunk + n) of a xorb served from decoded bytes through device tables "
           "(chunk addresses, serialized ends); rejected unless every chunk lies in a registered buffer")
      .def("start", &HbmSeeder::start)
      .def("stop", [](HbmSeeder& s) {
        py::gil_scoped_release nogil;
        s.stop();
      })
      .def_property_readonly("port", &HbmSeeder::port)
      .def("__len__", &HbmSeeder::count)
      .def("stats", [](const HbmSeeder& s) {
        auto st = s.stats();
        py::dict d;
        d["active_peers"] = st.active_peers;
        d["total_peers"] = st.total_peers;
        d["chunks_served"] = st.chunks_served;
        d["chunk_units"] = st.chunk_units;
        d["bytes_served"] = st.bytes_served;
        d["not_found"] = st.not_found;
        d["rejected"] = st.rejected;
        d["lookup_s"] = double(st.lookup_ns) / 1e9;
        d["wait_s"] = double(st.wait_ns) / 1e9;
        d["send_s"] = double(st.send_ns) / 1e9;
        d["resident_runs"] = s.resident_runs();
        return d;
      });
}
