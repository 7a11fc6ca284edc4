// rt_stage.hpp — where the inputs and outputs of one batch query sit in the context's staging
// buffer (rt_capi_queries.cpp).  The layout rule and nothing else: plain C++, no HIP, so the host
// test (tests/stage/stage_main.cpp) compiles it alone.
#pragma once

#include <cstddef>

namespace rtamd {

// One array of a query.  An input is copied host -> device before the launch, an output device ->
// host after it.  bytes == 0: an output that was not requested; it takes no space.
struct StageItem {
    const void* src = nullptr;  // input: the host bytes
    void* dst = nullptr;        // output: the host array
    size_t bytes = 0;
    size_t align = 8;   // of the element type: 8 for doubles and int32 pairs, 1 for bytes
    size_t offset = 0;  // set by layout()
};

// The items of one query in the order the caller declares them (at most kMaxItems).  layout()
// places them back to back in that order, except that the items aligned below 8 go last, after
// every other one.  The size of an 8-aligned item is a multiple of 8 (n doubles, n int32 pairs),
// so each of them sits at a multiple of 8 whatever n is, nothing is padded, and the total is the
// sum of the sizes.
struct StagePlan {
    static constexpr int kMaxItems = 8;
    StageItem item[kMaxItems];
    int count = 0;
    size_t total = 0;

    int input(const void* host, size_t bytes) {
        item[count].src = host;
        item[count].bytes = bytes;
        return count++;
    }
    int output(void* host, size_t bytes, size_t align = 8) {
        item[count].dst = host;
        item[count].bytes = bytes;
        item[count].align = align;
        return count++;
    }

    // An array the query continues in place: an output that is also an input when `read` is set.
    int inout(void* host, size_t bytes, bool read, size_t align = 8) {
        item[count].src = read ? host : nullptr;
        return output(host, bytes, align);
    }

    // kShort and kBytesFirst exist for the host test's mutants only (an item one byte into its
    // predecessor; the byte-sized items placed before the others).
    template <bool kShort = false, bool kBytesFirst = false>
    size_t layout() {
        size_t at = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (int i = 0; i < count; ++i) {
                StageItem& it = item[i];
                if ((it.align >= 8) != ((pass == 0) != kBytesFirst)) continue;
                it.offset = (kShort && it.bytes && at) ? at - 1 : at;
                at = it.offset + it.bytes;
            }
        return total = at;
    }
};

}  // namespace rtamd
