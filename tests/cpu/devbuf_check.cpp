// Host-only check of palace_amd/csrc/pa_devbuf.hpp: the two device functions are replaced by counting stand-ins, so every
// allocation and every release is seen here.  g++ -std=c++17 -I palace_amd/csrc; exit status 0: all checks hold.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <stdexcept>
#include <type_traits>
#include <utility>

#include "pa_devbuf.hpp"

namespace {
std::map<void *, int> g_freed;  // pointer handed out -> times released
int g_allocs = 0;
int g_fail_at = -1;  // the allocation with this number throws (-1: none)
int g_failed = 0;

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                      \
    }                                                                  \
  } while (0)

int freed(const void *p) { return g_freed.at(const_cast<void *>(p)); }
int total_freed() {
  int n = 0;
  for (const auto &kv : g_freed) n += kv.second;
  return n;
}
int64_t live() { return pa::g_dev_buffers_live.load(); }
}  // namespace

namespace pa {
void *dev_malloc_bytes(size_t bytes) {
  if (g_allocs == g_fail_at) throw std::runtime_error("allocation failed");
  g_allocs++;
  void *p = std::malloc(bytes);
  g_freed[p] = 0;  // (kept until the end of the program, so no address is handed out twice)
  return p;
}
void dev_free_bytes(void *p) noexcept { g_freed.at(p)++; }
}  // namespace pa

using pa::DevBuf;
using pa::Ref;

static_assert(sizeof(DevBuf<double>) == sizeof(double *), "DevBuf holds one pointer and nothing else");
static_assert(!std::is_copy_constructible<DevBuf<int>>::value && !std::is_copy_assignable<DevBuf<int>>::value, "move-only");
static_assert(!std::is_convertible<DevBuf<int> &&, int *>::value, "a temporary must be given an owner");
static_assert(std::is_convertible<const DevBuf<int> &, int *>::value, "an lvalue reads as its pointer");

// four arrays whose set-up can fail part of the way
struct Model {
  DevBuf<int> a, b;
  DevBuf<double> c, d;
  void setup() {
    a = pa::dev_alloc<int>(3);
    b = pa::dev_alloc<int>(3);
    c = pa::dev_alloc<double>(3);
    d = pa::dev_alloc<double>(3);
  }
};

struct Counted {
  static int deleted;
  int refcount = 0;
  ~Counted() { deleted++; }
};
int Counted::deleted = 0;

int main() {
  const int64_t live0 = live();
  {  // move construction
    DevBuf<double> a = pa::dev_alloc<double>(4);
    double *const p = a;
    CHECK(p && a.get() == p && live() == live0 + 1);
    DevBuf<double> b(std::move(a));
    CHECK(!a && a.get() == nullptr && b.get() == p && freed(p) == 0);
    {
      DevBuf<double> c(std::move(b));
      CHECK(c.get() == p && freed(p) == 0);
    }
    CHECK(freed(p) == 1 && live() == live0);
  }
  CHECK(total_freed() == 1);
  {  // move assignment onto a full buffer
    DevBuf<int> a = pa::dev_alloc<int>(2), b = pa::dev_alloc<int>(0);  // (zero entries: still an allocation of its own)
    int *const pa_ = a, *const pb = b;
    CHECK(pa_ != pb && live() == live0 + 2);
    a = std::move(b);
    CHECK(freed(pa_) == 1 && freed(pb) == 0 && a.get() == pb && !b && live() == live0 + 1);
    a = pa::dev_alloc<int>(5);  // the re-upload idiom: the old array goes, the new one stays
    CHECK(freed(pb) == 1 && live() == live0 + 1);
    int *const pc = a;
    DevBuf<int> &self = a;
    a = std::move(self);  // self-move: nothing released, nothing lost
    CHECK(a.get() == pc && freed(pc) == 0 && live() == live0 + 1);
    a.reset();
    CHECK(!a && freed(pc) == 1 && live() == live0);
    a.reset();  // (an empty buffer: no call)
    CHECK(freed(pc) == 1 && live() == live0);
  }
  CHECK(total_freed() == 4 && live() == live0);
  {  // release hands the pointer over
    DevBuf<double> a = pa::dev_alloc<double>(1);
    double *const p = a.release();
    CHECK(p && !a && freed(p) == 0 && live() == live0);
  }
  CHECK(total_freed() == 4 && live() == live0);
  {  // a set-up that throws after its second allocation
    const int before = g_allocs, freed_before = total_freed();
    void *pa0 = nullptr, *pb0 = nullptr;
    bool thrown = false;
    try {
      Model m;
      g_fail_at = before + 2;
      try {
        m.setup();
      } catch (...) {
        pa0 = m.a.get(), pb0 = m.b.get();
        CHECK(pa0 && pb0 && !m.c && !m.d && live() == live0 + 2);
        throw;
      }
    } catch (const std::runtime_error &) {
      thrown = true;
    }
    g_fail_at = -1;
    CHECK(thrown && g_allocs == before + 2 && total_freed() == freed_before + 2 && freed(pa0) == 1 && freed(pb0) == 1 &&
          live() == live0);
    Model ok;  // ... and one that does not: all four, once each
    ok.setup();
    CHECK(live() == live0 + 4);
  }
  CHECK(total_freed() == 10 && live() == live0);
  for (const auto &kv : g_freed) CHECK(kv.second <= 1);
  for (int order = 0; order < 2; order++) {  // two holders released in either order
    Counted::deleted = 0;
    Counted *obj = new Counted;
    Ref<Counted> first(obj);
    Ref<Counted> second = first;
    CHECK(obj->refcount == 2 && second.get() == obj);
    (order == 0 ? first : second) = Ref<Counted>();
    CHECK(Counted::deleted == 0 && obj->refcount == 1);
    (order == 0 ? second : first) = Ref<Counted>();
    CHECK(Counted::deleted == 1);
  }
  {  // an object whose creator keeps a reference without a handle (the pa_geom pattern)
    Counted::deleted = 0;
    Counted *obj = new Counted;
    obj->refcount = 1;
    {
      Ref<Counted> h(obj);
      Ref<Counted> moved(std::move(h));
      CHECK(obj->refcount == 2 && !h.get());
      h = moved;  // copy assignment
      CHECK(obj->refcount == 3);
    }
    CHECK(Counted::deleted == 0 && obj->refcount == 1);
    Ref<Counted>::drop(obj);
    CHECK(Counted::deleted == 1);
  }
  for (auto &kv : g_freed) std::free(kv.first);
  if (g_failed) return 1;
  std::printf("devbuf_check: all checks hold\n");
  return 0;
}
