// Host driver of the resource owners (csrc/polar_own.hpp) for tests/test_own_host.py, linked against tests/own/fake_hip.cpp.
// stdin: one command per line; stdout: one line of integers per command.  "live" = objects the fake runtime still holds:
// device blocks, pinned blocks, events, streams.
//   caps n...      per n, a fresh DBuf<double>: cap after ensure(n) | allocations it took | allocations of a second ensure(n)
//                  | 1 if ensure(smaller) kept the block
//   scope          live inside a scope that holds one owner of each kind (the Stream three times, once per way to make one)
//                  ... then live after it
//   release        the same with release() on each before the scope ends: live after the releases, live after the scope
//   vector count   `count` PinBuf<int> + Event pairs pushed into two vectors that reallocate on the way: live with them,
//                  1 if every element still holds what it was given, live after
//   moves          1 per check: a moved-from owner is empty and the target holds the block (construction and assignment,
//                  each kind), then live at the end
//   fail           DBuf and PinBuf in turn: a growth whose allocation fails: 1 if HipError was thrown | p == nullptr | cap |
//                  live blocks of that kind | cap after a later ensure; then live after both have gone
//   borrow         live streams while a Stream lends a stream made elsewhere | after the Stream has gone | after its maker
//                  destroyed it; then the same through release()
//   poison         first and last byte of a fresh DBuf<unsigned char> of 100 (0x7F with POLAR_POISON=1 in the environment)
//   errors         one exception of each class the entry points tell apart (InputError, Unsupported, NoDevice, HipError, any other
//                  std::exception), each on a line: the code error_code gives it, then its message
//   live           live
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "polar_own.hpp"

extern "C" {
long fake_live(int kind);
long fake_allocs(void);
void fake_fail_nth(long n);
}

template <class T>
constexpr bool move_only = !std::is_copy_constructible<T>::value && !std::is_copy_assignable<T>::value &&
                           std::is_nothrow_move_constructible<T>::value && std::is_nothrow_move_assignable<T>::value;
static_assert(move_only<DBuf<double>> && move_only<DBuf<int>>, "DBuf is move-only");
static_assert(move_only<PinBuf<int>>, "PinBuf is move-only");
static_assert(move_only<Event>, "Event is move-only");
static_assert(move_only<Stream>, "Stream is move-only");
static_assert(std::is_convertible<Event, hipEvent_t>::value && std::is_convertible<Stream, hipStream_t>::value, "launch sites read them as handles");

namespace {
void print_live(const char *end = "\n") { printf("%ld %ld %ld %ld%s", fake_live(0), fake_live(1), fake_live(2), fake_live(3), end); }

template <class B>
void fail_case(int kind) {
  B b;
  b.ensure(10);
  bool thrown = false;
  fake_fail_nth(1);
  try { b.ensure(1000); } catch (const HipError &) { thrown = true; }
  printf("%d %d %zu %ld ", thrown ? 1 : 0, b.p == nullptr ? 1 : 0, b.cap, fake_live(kind));
  b.ensure(1000);
  b.p[999] = 1;   // (the block is there and as long as it says)
  printf("%zu ", b.cap);
}
}  // namespace

int main() {
  char cmd[32];
  while (scanf("%31s", cmd) == 1) {
    if (!strcmp(cmd, "caps")) {
      int count;
      if (scanf("%d", &count) != 1) return 2;
      for (int k = 0; k < count; k++) {
        long long n;
        if (scanf("%lld", &n) != 1 || n < 0) return 2;
        DBuf<double> b;
        const long a0 = fake_allocs();
        b.ensure((size_t)n);
        const long a1 = fake_allocs();
        if (b.cap) { b.p[0] = 1.0; b.p[b.cap - 1] = 2.0; }
        const double *was = b.p;
        b.ensure((size_t)n);
        const long a2 = fake_allocs();
        b.ensure((size_t)n / 2);
        b.ensure(b.cap);
        printf("%zu %ld %ld %d\n", b.cap, a1 - a0, a2 - a1, (b.p == was && fake_allocs() == a2) ? 1 : 0);
      }
    } else if (!strcmp(cmd, "scope") || !strcmp(cmd, "release")) {
      {
        DBuf<double> d; PinBuf<int> p; Event e0, e1; Stream s0, s1, s2;
        d.ensure(100); p.ensure(100); e0.create(); e1.create(hipEventDisableTiming);
        s0.create(); s1.create(hipStreamNonBlocking); s2.create(hipStreamNonBlocking, 0);
        d.p[99] = 1.0; p.p[99] = 1;
        if (cmd[0] == 's') print_live(" ");
        else {
          d.release(); p.release(); e0.release(); e1.release(); s0.release(); s1.release(); s2.release();
          d.release(); e0.release();   // (a second release finds nothing)
          if (d.p || d.cap || p.p || p.cap || (hipEvent_t)e0 || (hipStream_t)s0) return 3;
          print_live(" ");
        }
      }
      print_live();
    } else if (!strcmp(cmd, "vector")) {
      int count;
      if (scanf("%d", &count) != 1 || count < 0) return 2;
      {
        std::vector<PinBuf<int>> bufs; std::vector<Event> evs;
        std::vector<int *> pp; std::vector<hipEvent_t> ee;
        for (int k = 0; k < count; k++) {
          PinBuf<int> p; Event e;
          p.ensure(16); e.create(hipEventDisableTiming);
          p.p[0] = k;
          pp.push_back(p.p); ee.push_back(e);
          bufs.push_back(std::move(p)); evs.push_back(std::move(e));
          if (p.p || p.cap || (hipEvent_t)e) return 3;
        }
        bool same = true;
        for (int k = 0; k < count; k++) same = same && bufs[k].p == pp[k] && bufs[k].p[0] == k && (hipEvent_t)evs[k] == ee[k];
        print_live(" ");
        printf("%d ", same ? 1 : 0);
      }
      print_live();
    } else if (!strcmp(cmd, "moves")) {
      {
        DBuf<double> a; a.ensure(10); double *ap = a.p; const size_t ac = a.cap;
        DBuf<double> b(std::move(a));
        printf("%d ", (!a.p && !a.cap && b.p == ap && b.cap == ac) ? 1 : 0);
        DBuf<double> c; c.ensure(5);
        c = std::move(b);   // (lets go of its own block)
        printf("%d ", (!b.p && !b.cap && c.p == ap && c.cap == ac && fake_live(0) == 1) ? 1 : 0);
        PinBuf<int> p; p.ensure(10); int *pp = p.p;
        PinBuf<int> q(std::move(p)), r; r.ensure(3);
        r = std::move(q);
        printf("%d ", (!p.p && !q.p && !q.cap && r.p == pp && r.cap == 10 && fake_live(1) == 1) ? 1 : 0);
        Event e; e.create(); hipEvent_t eh = e;
        Event f(std::move(e)), g; g.create();
        g = std::move(f);
        printf("%d ", (!(hipEvent_t)e && !(hipEvent_t)f && (hipEvent_t)g == eh && fake_live(2) == 1) ? 1 : 0);
        Stream s; s.create(); hipStream_t sh = s;
        Stream t(std::move(s)), u; u.create();
        u = std::move(t);
        printf("%d ", (!(hipStream_t)s && !(hipStream_t)t && (hipStream_t)u == sh && fake_live(3) == 1) ? 1 : 0);
      }
      print_live();
    } else if (!strcmp(cmd, "fail")) {
      fail_case<DBuf<double>>(0);
      fail_case<PinBuf<double>>(1);
      print_live();
    } else if (!strcmp(cmd, "borrow")) {
      for (int how = 0; how < 2; how++) {
        hipStream_t foreign = nullptr;
        if (hipStreamCreate(&foreign) != hipSuccess) return 3;
        {
          Stream s;
          s.create();
          s.borrow(foreign);   // (its own stream goes, the lent one stands in)
          if ((hipStream_t)s != foreign) return 3;
          printf("%ld ", fake_live(3));
          if (how) { s.release(); if ((hipStream_t)s) return 3; }
        }
        printf("%ld ", fake_live(3));
        if (hipStreamDestroy(foreign) != hipSuccess) return 3;
        printf("%ld%s", fake_live(3), how ? "\n" : " ");
      }
    } else if (!strcmp(cmd, "poison")) {
      DBuf<unsigned char> b;
      b.ensure(100);
      printf("%d %d\n", (int)b.p[0], (int)b.p[b.cap - 1]);
    } else if (!strcmp(cmd, "errors")) {
      for (int k = 0; k < 5; k++) {
        std::string msg = "stale";
        int code = 0;
        try {
          if (k == 0) throw polar::InputError("bad input");
          if (k == 1) throw polar::Unsupported("not offered");
          if (k == 2) throw NoDevice();
          if (k == 3) throw HipError("hipFoo failed");
          throw std::logic_error("out of order");
        } catch (...) { code = error_code(msg); }
        printf("%d %s\n", code, msg.c_str());
      }
    } else if (!strcmp(cmd, "live")) {
      print_live();
    } else {
      fprintf(stderr, "unknown command %s\n", cmd);
      return 2;
    }
  }
  return (fake_live(0) || fake_live(1) || fake_live(2) || fake_live(3)) ? 4 : 0;
}
