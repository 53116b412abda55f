// Memory a call is handed in one piece and cuts into typed arrays: the context's scratch (api.hip) and
// every caller workspace.  One function per workspace names its pieces with Carver::take; run without a
// base it gives the size (the explainn_*_workspace_bytes exports), run on the caller's pointer it gives the
// addresses, so the two cannot drift apart.  This is the only place in csrc/ that rounds to 256 bytes.
#pragma once
#include "common.h"

namespace {

struct Carver {
    int64_t off = 0;
    char* base = nullptr;
    explicit Carver(void* ws = nullptr) : base(static_cast<char*>(ws)) {}
    // the next piece: `count` elements of T, 256-byte aligned from the base
    template <typename T>
    void take(T** p, int64_t count) {
        off = (off + 255) & ~int64_t(255);
        if (base) *p = reinterpret_cast<T*>(base + off);
        off += count * (int64_t)sizeof(T);
    }
    // the size of everything taken, the last piece rounded up too
    int64_t bytes() const { return (off + 255) & ~int64_t(255); }
};

// What every entry point asks of its caller's workspace: non-null, `align`-byte aligned (1: any address),
// at least `need` bytes.
bool workspace_ok(const char* who, const void* ws, int64_t given, int64_t need, int align) {
    if (ws && given >= need && reinterpret_cast<uintptr_t>(ws) % (uintptr_t)align == 0) return true;
    explainn_set_error("%s: workspace of %lld bytes given, %lld needed, %d-byte aligned", who, (long long)given,
                       (long long)need, align);
    return false;
}

}  // namespace
