// The owners of sorobn_amd/csrc/device_mem.h against a fake HIP runtime (tools/fake_hip: malloc-backed handles and a ledger of every
// create and release), on the host:
//   g++ -std=c++17 -fsanitize=address,undefined -I tools/fake_hip tools/device_mem_sim.cpp -o device_mem_sim && ./device_mem_sim
// Exits 0 when every check holds; the first that does not prints its line and exits 1 (tests/test_device_mem_host.py).
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "../sorobn_amd/csrc/device_mem.h"

using namespace mibn;
using fake_hip::ledger;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

// every handle handed out since the last reset has been released exactly once, and nothing else was released
static bool all_released_once() {
    for (const auto &kv : ledger().handles)
        if (kv.second.created != 1 || kv.second.released != 1) return false;
    return ledger().unknown_releases == 0;
}
static long n_handles(fake_hip::Kind k) {
    long n = 0;
    for (const auto &kv : ledger().handles) n += kv.second.kind == k;
    return n;
}
static const fake_hip::Handle &handle(const void *p) { return ledger().handles.at(const_cast<void *>(p)); }

struct OneOfEach {  // declared like mibn_ctx: the stream first, so that it goes last
    Stream stream, planning;
    DevBuf<double> dev;
    PinnedBuf pin;
    Event timing, order;
    // creates everything in a fixed order, stopping at the first failure like a function full of HIP_TRY
    hipError_t fill() {
        if (hipError_t e = stream.ensure(hipStreamNonBlocking)) return e;
        if (hipError_t e = planning.ensure(hipStreamNonBlocking, -1)) return e;
        if (hipError_t e = dev.ensure(100)) return e;
        if (hipError_t e = dev.ensure(5000)) return e;  // (grows: the second device allocation)
        if (hipError_t e = pin.ensure(100)) return e;
        if (hipError_t e = timing.ensure()) return e;
        if (hipError_t e = order.ensure(hipEventDisableTiming)) return e;
        return hipSuccess;
    }
};
constexpr long kFillCreates = 7;

static void empty_owners_make_no_calls() {
    fake_hip::reset();
    {
        DevBuf<int> d;
        PinnedBuf p;
        Event e;
        Stream s;
        OneOfEach all;
        CHECK(!d.get() && d.cap() == 0 && !p.get() && p.cap() == 0 && !e.get() && !s.get());
        CHECK(d.release() == hipSuccess && p.release() == hipSuccess && e.release() == hipSuccess && s.release() == hipSuccess);
        DevBuf<int> d2(std::move(d));
        d = std::move(d2);
    }
    CHECK(ledger().calls == 0);
}

static void growth_policies() {
    fake_hip::reset();
    {
        DevBuf<double> d;
        CHECK(d.ensure(0) == hipSuccess && ledger().calls == 0);  // (nothing asked for, nothing allocated)
        CHECK(d.ensure(1000) == hipSuccess);
        CHECK(ledger().calls == 1 && d.cap() == 1000 + 500 + 1024 && handle(d.get()).bytes == d.cap() * sizeof(double));
        const void *first = d.get();
        for (size_t need : {size_t(1), size_t(1000), d.cap()}) CHECK(d.ensure(need) == hipSuccess && ledger().calls == 1 && d.get() == first);
        const size_t need = d.cap() + 1;  // above capacity: one free, one allocation
        CHECK(d.ensure(need) == hipSuccess);
        CHECK(ledger().calls == 3 && handle(first).released == 1 && d.get() != first);
        CHECK(d.cap() == need + need / 2 + 1024 && handle(d.get()).bytes == d.cap() * sizeof(double));
        CHECK(d.reset(7) == hipSuccess && d.cap() == 7 && handle(d.get()).bytes == 7 * sizeof(double) && ledger().calls == 5);
        CHECK(d.reset(7) == hipSuccess && ledger().calls == 7);  // (reset always allocates afresh)
        CHECK(d.release() == hipSuccess && !d.get() && d.cap() == 0 && ledger().calls == 8);

        PinnedBuf p;
        CHECK(p.ensure(10000) == hipSuccess);
        CHECK(p.cap() == 10000 + 2500 + 4096 && handle(p.get()).bytes == p.cap() && handle(p.get()).flags == hipHostMallocDefault);
        const long before = ledger().calls;
        CHECK(p.ensure(p.cap()) == hipSuccess && ledger().calls == before);
        const void *pin0 = p.get();
        const size_t more = p.cap() + 1;
        CHECK(p.ensure(more) == hipSuccess && ledger().calls == before + 2 && handle(pin0).released == 1 && p.cap() == more + more / 4 + 4096);
        // a pinned pointer that lives outside an owner for a while (ProgBuf::data)
        PinnedBuf q;
        CHECK(q.reset(64) == hipSuccess && q.cap() == 64);
        char *raw = q.detach();
        CHECK(raw && !q.get() && q.cap() == 0 && handle(raw).released == 0);
        CHECK(PinnedBuf::adopt(raw).release() == hipSuccess && handle(raw).released == 1);
        CHECK(PinnedBuf::adopt(nullptr).release() == hipSuccess);

        Event t, o;
        CHECK(t.ensure() == hipSuccess && o.ensure(hipEventDisableTiming) == hipSuccess);
        CHECK(handle(t.get()).flags == hipEventDefault && handle(o.get()).flags == hipEventDisableTiming);
        const hipEvent_t t0 = t.get();
        const long ev_calls = ledger().calls;
        CHECK(t.ensure() == hipSuccess && t.get() == t0 && ledger().calls == ev_calls);  // (created once)
        Stream s, hi;
        CHECK(s.ensure(hipStreamNonBlocking) == hipSuccess && hi.ensure(hipStreamNonBlocking, -2) == hipSuccess);
        CHECK(handle(s.get()).flags == hipStreamNonBlocking && handle(s.get()).priority == 0 && handle(hi.get()).priority == -2);
        const long st_calls = ledger().calls;
        CHECK(s.ensure(hipStreamNonBlocking) == hipSuccess && hi.ensure(hipStreamNonBlocking, -2) == hipSuccess && ledger().calls == st_calls);
    }
    CHECK(all_released_once());
}

template <class Owner, class Make>
static void moves_of(Make make) {
    fake_hip::reset();
    {
        Owner a, b;
        CHECK(make(a) == hipSuccess && make(b) == hipSuccess);
        const auto ha = a.get(), hb = b.get();
        Owner c(std::move(a));  // move construction: the source is empty, nothing is released
        CHECK(!a.get() && c.get() == ha && handle(ha).released == 0);
        b = std::move(c);  // move assignment over a live owner: what it held is released, once
        CHECK(!c.get() && b.get() == ha && handle(hb).released == 1 && handle(ha).released == 0);
        Owner &same = b;
        b = std::move(same);  // self move assignment keeps the handle
        CHECK(b.get() == ha && handle(ha).released == 0);
        a = std::move(b);  // into an empty owner
        CHECK(a.get() == ha && !b.get() && handle(ha).released == 0);
    }
    CHECK(ledger().handles.size() == 2 && all_released_once());
}

static void failure_at_each_creation() {
    for (long k = 1; k <= kFillCreates + 1; ++k) {  // (the last round: no failure at all)
        fake_hip::reset();
        ledger().fail_at = k;
        {
            OneOfEach all;
            const hipError_t e = all.fill();
            CHECK((e != hipSuccess) == (k <= kFillCreates));
            CHECK((long)ledger().handles.size() == (k <= kFillCreates ? k - 1 : kFillCreates));
            if (e == hipSuccess) CHECK(n_handles(fake_hip::kStream) == 2 && n_handles(fake_hip::kDevice) == 2 && n_handles(fake_hip::kPinned) == 1 && n_handles(fake_hip::kEvent) == 2);
            // an owner whose creation failed is empty, not half-made
            if (k == 3 || k == 4) CHECK(!all.dev.get() && all.dev.cap() == 0);
            if (k == 5) CHECK(!all.pin.get() && all.pin.cap() == 0);
            // the streams outlive everything created after them: nothing of theirs is released before the struct goes
            if (k > 1) CHECK(handle(all.stream.get()).released == 0);
        }
        CHECK(all_released_once());
    }
}

int main() {
    empty_owners_make_no_calls();
    growth_policies();
    moves_of<DevBuf<float>>([](DevBuf<float> &d) { return d.ensure(10); });
    moves_of<PinnedBuf>([](PinnedBuf &p) { return p.ensure(10); });
    moves_of<Event>([](Event &e) { return e.ensure(); });
    moves_of<Stream>([](Stream &s) { return s.ensure(hipStreamNonBlocking); });
    failure_at_each_creation();
    fake_hip::reset();
    std::puts("device_mem_sim: ok");
    return 0;
}
