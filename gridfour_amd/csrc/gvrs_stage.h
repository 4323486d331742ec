// gvrs_stage.h -- the staging of ONE host-form call, stated once: the call declares its parts in order (an input with its host
// pointer and byte count, an output, a part that is both, a device-only part), begin() lays them out with a Carve, makes the ONE
// staging buffer hold them, marks it in use and enqueues the inputs and the zeroing; ptr<T>(part) is a part in device memory;
// fetch() copies an output, or a prefix of it, home now; flush() enqueues the outputs not fetched yet and synchronises once;
// end() is flush() and gives the buffer back, as the destructor does on every other way out.  A part's size is written in its
// declaration and nowhere else.  Plain C++, no HIP include: what touches the device is the Dev the stage is built on (StageDev of
// gvrs_api_internal.h; the host test's copies with memcpy):
//     typedef ... Status;                                 Status() is success, anything else ends the call
//     bool &busy();                                       the buffer's in-use mark
//     Status reserve(size_t bytes, unsigned char *&base); the buffer holds `bytes` bytes; base = its address
//     Status toDevice(void *d, const void *h, size_t n);  Status toHost(void *h, const void *d, size_t n);
//     Status zero(void *d, size_t n);                     Status sync();
//     Status refuse(const char *why);                     the status of a stage that may not begin; records why
#pragma once

#include <cstddef>

#include "gvrs_carve.h"

enum : unsigned {
    STAGE_IN = 1,        // copied to the device when the stage begins
    STAGE_OUT = 2,       // copied home by flush() / end(), unless fetched before
    STAGE_HELD = 4,      // copied home by fetch() alone: the call learns from other outputs how much of it counts.  It takes its
                         // room without a host pointer too: the device writes it whether or not the caller has room for any of it
    STAGE_ZERO = 8,      // zeroed on the stream when the stage begins
    STAGE_LOCAL = 16     // no host side
};

constexpr int STAGE_MAX_PARTS = 2 * 16 + 12;            // GF_MAX_ELEMS arrays twice and a dozen single parts

template <class Dev>
class Stage {
public:
    typedef typename Dev::Status Status;
    explicit Stage(Dev d) : dev(d) {}
    Stage(const Stage &) = delete;
    ~Stage() { release(); }

    // The declarations: each returns the part's number.  A part of some bytes without a host pointer, where it should have one, is
    // ABSENT (an output the caller did not ask for): it takes no room, nothing is copied and ptr() reads as null.  A part of 0 bytes
    // is never absent: it shares its offset with the next one (an empty batch still hands the device forms pointers that are not
    // null).  slack: readable bytes behind an input (the kernels read whole words past a blob's end).
    int add(void *host, size_t bytes, unsigned flags, size_t slack = 0)
    {
        if (n == STAGE_MAX_PARTS) {
            over = true;                                // (begin() refuses; the number returned is never used)
            return 0;
        }
        Part &p = part[n];
        p.host = host, p.flags = flags, p.done = false;
        p.absent = !host && bytes && !(flags & (STAGE_LOCAL | STAGE_HELD));
        p.bytes = p.absent ? 0 : bytes;
        p.at = lay.add(p.absent ? 0 : bytes + slack);
        return n++;
    }
    int in(const void *host, size_t bytes, size_t slack = 0) { return add(const_cast<void *>(host), bytes, STAGE_IN, slack); }
    int out(void *host, size_t bytes) { return add(host, bytes, STAGE_OUT); }
    int inout(void *host, size_t bytes) { return add(host, bytes, STAGE_IN | STAGE_OUT); }
    int held(void *host, size_t bytes) { return add(host, bytes, STAGE_HELD); }
    int local(size_t bytes, bool zeroed = false) { return add(nullptr, bytes, STAGE_LOCAL | (zeroed ? STAGE_ZERO : 0u)); }

    size_t total() const { return lay.total; }

    Status begin()
    {
        if (over) return dev.refuse("stage: more parts than the table holds");
        if (dev.busy()) return dev.refuse("stage: the staging buffer is in use by a call that has not ended");
        Status s = dev.reserve(lay.total, base);
        if (s != Status()) return s;
        dev.busy() = mine = true;
        for (int i = 0; i < n; i++)
            if ((part[i].flags & STAGE_IN) && part[i].bytes && (s = dev.toDevice(base + part[i].at, part[i].host, part[i].bytes)) != Status()) return s;
        for (int i = 0; i < n; i++) {                   // neighbours that are zeroed: one fill (parts are laid out back to back)
            if (!(part[i].flags & STAGE_ZERO) || !part[i].bytes) continue;
            int j = i;
            while (j + 1 < n && (part[j + 1].flags & STAGE_ZERO)) j++;
            if ((s = dev.zero(base + part[i].at, part[j].at + part[j].bytes - part[i].at)) != Status()) return s;
            i = j;
        }
        return Status();
    }

    template <class T> T *ptr(int i) const { return part[i].absent ? nullptr : reinterpret_cast<T *>(base + part[i].at); }
    void ptrs(const int *which, int count, void **out) const { for (int k = 0; k < count; k++) out[k] = ptr<void>(which[k]); }

    // an output's first `bytes` bytes (all of it by default) to its host pointer, enqueued now; flush() passes it over afterwards
    Status fetch(int i, size_t bytes = ~(size_t)0)
    {
        Part &p = part[i];
        p.done = true;
        if (bytes > p.bytes) bytes = p.bytes;
        return bytes && p.host ? dev.toHost(p.host, base + p.at, bytes) : Status();
    }

    Status flush()
    {
        Status s = Status();
        for (int i = 0; i < n && s == Status(); i++)
            if ((part[i].flags & STAGE_OUT) && !part[i].done) s = fetch(i);
        return s != Status() ? s : dev.sync();
    }

    Status end()
    {
        const Status s = flush();
        release();
        return s;
    }

private:
    struct Part {
        void *host;
        size_t bytes, at;
        unsigned flags;
        bool absent, done;
    };
    void release() { if (mine) dev.busy() = mine = false; }
    Dev dev;
    Carve lay;
    Part part[STAGE_MAX_PARTS];
    unsigned char *base = nullptr;
    int n = 0;
    bool over = false, mine = false;
};
