// Host check of csrc/workspace.hpp's Carver (tests/test_workspace.py compiles this under ASan + UBSan and runs it):
// pseudo-random layouts measured and carved by the same code, the overflow rules, and a layout nested in another.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "workspace.hpp"

namespace {

struct alignas(16) Wide {
  unsigned char b[16];
};

struct Req {
  int size;  // 1, 2, 4, 8, 16
  size_t count, align;
};

int g_failures = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      ++g_failures;                              \
      std::printf("FAIL %s: ", #cond);           \
      std::printf(__VA_ARGS__);                  \
      std::printf("\n");                         \
    }                                            \
  } while (0)

uintptr_t take_req(mq::Carver& c, const Req& r) {
  switch (r.size) {
    case 1: return reinterpret_cast<uintptr_t>(c.take<uint8_t>(r.count, r.align));
    case 2: return reinterpret_cast<uintptr_t>(c.take<uint16_t>(r.count, r.align));
    case 4: return reinterpret_cast<uintptr_t>(c.take<uint32_t>(r.count, r.align));
    case 8: return reinterpret_cast<uintptr_t>(c.take<uint64_t>(r.count, r.align));
    default: return reinterpret_cast<uintptr_t>(c.take<Wide>(r.count, r.align));
  }
}

// A stage's layout function: takes reqs[lo, hi) in order and records where each landed.
void inner_layout(mq::Carver& c, const std::vector<Req>& reqs, size_t lo, size_t hi, std::vector<uintptr_t>& at) {
  for (size_t i = lo; i < hi; ++i) at.push_back(take_req(c, reqs[i]));
}

// A composite's layout function: its own arrays around a sub-stage's layout on the same carver (NMS inside the RPN).
void outer_layout(mq::Carver& c, const std::vector<Req>& reqs, size_t lo, size_t hi, std::vector<uintptr_t>& at) {
  for (size_t i = 0; i < lo; ++i) at.push_back(take_req(c, reqs[i]));
  inner_layout(c, reqs, lo, hi, at);
  for (size_t i = hi; i < reqs.size(); ++i) at.push_back(take_req(c, reqs[i]));
}

void check_sequence(int seq, const std::vector<Req>& reqs, size_t lo, size_t hi) {
  // (a), (e): the same code measures and carves
  mq::Carver m;
  std::vector<uintptr_t> off;
  outer_layout(m, reqs, lo, hi, off);
  const size_t used = m.used();
  CHECK(!m.fits(), "seq %d: a measuring carver never fits", seq);
  void* mem = nullptr;
  if (posix_memalign(&mem, 256, used ? used : 1) != 0) std::abort();
  const uintptr_t base = reinterpret_cast<uintptr_t>(mem);
  mq::Carver c(mem, used);
  std::vector<uintptr_t> ptr;
  outer_layout(c, reqs, lo, hi, ptr);
  CHECK(c.used() == used, "seq %d: used %zu measured, %zu carved", seq, used, c.used());
  CHECK(off.size() == reqs.size() && ptr.size() == reqs.size(), "seq %d: take count", seq);
  // (b): alignment, order, disjointness, containment; each range is written (ASan watches the allocation's end)
  uintptr_t end_prev = 0;
  for (size_t i = 0; i < reqs.size(); ++i) {
    const size_t bytes = reqs[i].count * (size_t)reqs[i].size;
    CHECK(ptr[i] - base == off[i], "seq %d take %zu: offset %zu measured, %zu carved", seq, i, (size_t)off[i],
          (size_t)(ptr[i] - base));
    CHECK(off[i] % reqs[i].align == 0 && ptr[i] % reqs[i].align == 0, "seq %d take %zu: align %zu", seq, i,
          reqs[i].align);
    CHECK(off[i] >= end_prev, "seq %d take %zu: overlaps the one before", seq, i);
    CHECK(off[i] < end_prev + reqs[i].align, "seq %d take %zu: more padding than the alignment asks", seq, i);
    CHECK(off[i] + bytes <= used, "seq %d take %zu: ends past used()", seq, i);
    end_prev = off[i] + bytes;
    if (off[i] + bytes <= used) std::memset(reinterpret_cast<void*>(ptr[i]), (int)(i + 1), bytes);
  }
  CHECK(end_prev == used, "seq %d: used() %zu is not the last array's end %zu", seq, used, (size_t)end_prev);
  for (size_t i = 0; i < reqs.size(); ++i) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(ptr[i]);
    const size_t bytes = reqs[i].count * (size_t)reqs[i].size;
    for (size_t k = 0; k < bytes && off[i] + bytes <= used; ++k)
      if (p[k] != (unsigned char)(i + 1)) {
        CHECK(false, "seq %d take %zu: byte %zu was overwritten by another range", seq, i, k);
        break;
      }
  }
  // (c): exactly used() bytes fit, one fewer does not
  CHECK(c.fits(), "seq %d: does not fit in used() = %zu bytes", seq, used);
  if (used > 0) {
    mq::Carver t(mem, used - 1);
    std::vector<uintptr_t> tmp;
    outer_layout(t, reqs, lo, hi, tmp);
    CHECK(!t.fits() && t.used() == used, "seq %d: fits in used() - 1 bytes", seq);
  }
  std::free(mem);
}

// (d): a byte count or an offset that would wrap size_t is a sticky failure, in both modes
template <class F>
void check_overflow(const char* name, F takes) {
  alignas(256) static unsigned char buf[256];
  for (int carving = 0; carving < 2; ++carving) {
    mq::Carver c = carving ? mq::Carver(buf, sizeof(buf)) : mq::Carver();
    takes(c);
    CHECK(!c.fits() && c.used() == SIZE_MAX, "%s (%s): fits %d used %zu", name, carving ? "carving" : "measuring",
          (int)c.fits(), c.used());
    c.take<uint8_t>(1);  // and stays one
    CHECK(!c.fits() && c.used() == SIZE_MAX, "%s (%s): the failure did not stick", name,
          carving ? "carving" : "measuring");
  }
}

}  // namespace

int main() {
  std::mt19937_64 rng(20240611);
  const int sizes[5] = {1, 2, 4, 8, 16};
  const int n_seq = 400;
  for (int seq = 0; seq < n_seq; ++seq) {
    std::vector<Req> reqs(1 + rng() % 12);
    for (Req& r : reqs) {
      r.size = sizes[rng() % 5];
      int lg = (int)(rng() % 9);  // align 1 ... 256, at least the element's own
      while (((size_t)1 << lg) < (size_t)r.size) ++lg;
      r.align = (size_t)1 << lg;
      const unsigned kind = (unsigned)(rng() % 8);
      r.count = kind == 0 ? 0 : kind < 5 ? 1 + rng() % 9 : 1 + rng() % 3000;
    }
    size_t lo = rng() % (reqs.size() + 1), hi = rng() % (reqs.size() + 1);
    if (lo > hi) std::swap(lo, hi);
    check_sequence(seq, reqs, lo, hi);
  }

  check_overflow("count * sizeof(T) wraps", [](mq::Carver& c) { c.take<uint64_t>(SIZE_MAX / 4); });
  check_overflow("offset + bytes wraps", [](mq::Carver& c) {
    c.take<uint8_t>(SIZE_MAX - 10, 1);
    c.take<uint8_t>(100, 1);
  });
  check_overflow("aligning the offset wraps", [](mq::Carver& c) {
    c.take<uint8_t>(SIZE_MAX - 10, 1);
    c.take<uint8_t>(0, 256);
  });
  check_overflow("align is no power of two", [](mq::Carver& c) { c.take<uint8_t>(4, 24); });
  check_overflow("align below alignof(T)", [](mq::Carver& c) { c.take<uint64_t>(4, 4); });
  {  // a carving carver's base must be 256-byte aligned
    alignas(256) static unsigned char buf[512];
    mq::Carver c(buf + 64, 256);
    c.take<uint8_t>(1);
    CHECK(!c.fits(), "a base at 64 mod 256 was accepted");
  }
  CHECK(mq::align256(0) == 0 && mq::align256(1) == 256 && mq::align256(256) == 256 && mq::align256(257) == 512,
        "align256");

  std::printf("%s: %d sequences, %d failures\n", g_failures ? "FAILED" : "ok", n_seq, g_failures);
  return g_failures ? 1 : 0;
}
