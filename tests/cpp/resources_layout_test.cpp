// The host-only pieces of tbraymarcherplugin_amd/csrc/tbrm_resources.h that state a layout or own memory: DeviceScratch (an empty
// guard never touches the device: move and destruction need none) and tbrm_resources::Residency's layers() / bytes() / address().
// Built with the address and undefined-behaviour sanitizers by tests/test_resources_layout.py; allocates nothing through HIP.
#include "../../tbraymarcherplugin_amd/csrc/tbrm_resources.h"

#include <cstdio>
#include <utility>

namespace tbrm_host {
int fail(int code, const char*, ...) { return code; } // (tbrm_api.cpp's is not linked here)
}

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

using Residency = tbrm_resources::Residency;

// `alloc` is host memory here and never dereferenced: address() only offsets it
static Residency residency(char* alloc, int lo, int hi, int wrap_src, size_t layer_bytes)
{
    Residency q;
    q.lo = lo; q.hi = hi; q.wrap_src = wrap_src; q.layer_bytes = layer_bytes; q.alloc = alloc;
    return q;
}

int main()
{
    {   // an empty guard: default, moved from, moved into, move-assigned, destroyed
        DeviceScratch a;
        CHECK(a.p == nullptr);
        DeviceScratch b(std::move(a));
        CHECK(a.p == nullptr && b.p == nullptr);
        DeviceScratch c;
        c = std::move(b);
        CHECK(b.p == nullptr && c.p == nullptr);
    }
    constexpr size_t L = 4096;
    constexpr int layers = 8;
    static char block[layers * L];
    char* const base = block;
    {   // a whole-volume handle: every layer, no wrap copy
        const Residency q = residency(base, 0, layers, -1, L);
        CHECK(q.layers() == 8 && q.bytes() == 8 * L);
        for (int l = 0; l < layers; ++l) CHECK(q.address(l) == base + (size_t) l * L);
        CHECK(q.address(-1) == nullptr && q.address(layers) == nullptr);
    }
    {   // the first slab: layers [0, 5) and a copy of the last layer behind them
        const Residency q = residency(base, 0, 5, layers - 1, L);
        CHECK(q.layers() == 6 && q.bytes() == 6 * L);
        for (int l = 0; l < 5; ++l) CHECK(q.address(l) == base + (size_t) l * L);
        CHECK(q.address(layers - 1) == base + 5 * L);
        CHECK(q.address(5) == nullptr && q.address(6) == nullptr && q.address(-1) == nullptr);
    }
    {   // the last slab: layers [3, 8) and a copy of layer 0 behind them
        const Residency q = residency(base, 3, layers, 0, L);
        CHECK(q.layers() == 6 && q.bytes() == 6 * L);
        for (int l = 3; l < layers; ++l) CHECK(q.address(l) == base + (size_t) (l - 3) * L);
        CHECK(q.address(0) == base + 5 * L);
        CHECK(q.address(1) == nullptr && q.address(2) == nullptr && q.address(layers) == nullptr);
    }
    {   // a middle slab: no wrap copy, nothing outside [lo, hi)
        const Residency q = residency(base, 2, 6, -1, L);
        CHECK(q.layers() == 4 && q.bytes() == 4 * L);
        CHECK(q.address(2) == base && q.address(5) == base + 3 * L && q.address(1) == nullptr && q.address(6) == nullptr && q.address(-1) == nullptr);
    }
    printf("failures=%d\n", failures);
    return failures ? 1 : 0;
}
