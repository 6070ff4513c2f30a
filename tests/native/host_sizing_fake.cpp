// host_sizing_fake.cpp -- the host-batch pipeline (swmi_api.cpp score_host_batch) on fake GPUs (fake_hip.cpp), at the sizes
// where a LATER score group's schedule has a larger granule than the first group's: the balanced schedule of the 2-bit packed
// entry cuts its middle at multiples of 4096 and gives the rest to the last middle granule, so a ragged tail group can carry a
// granule of up to steady + 4095 pairs where a full group divides evenly.  Every case runs on a FRESH context (swmi_shutdown,
// then swmi_init), so no buffer grown by an earlier call can hide a slot that is too small; the fake aborts on any copy or
// launch that leaves its device block.  The bad sizes are found from the schedule itself (swmi_host_granules_for), not
// hard-coded.  The fake launchers return the number in a pair's first four bytes, so every score vector must read 0, 1, 2, ...
// Built and run by tests/test_host_sizing_fake.py (g++, ASan + UBSan, no GPU).
//
//   host_sizing_fake group     SWMI_TEST_SCORE_GROUP set by the caller: the three entries at one group + the worst tail, the
//                              packed entry at several bad tails
//   host_sizing_fake small     a small group and SWMI_HOST_MIN_GRANULE set by the caller: many bad tails, all three entries
//   host_sizing_fake multi     swmi_score_batch_packed_multi on three fake GPUs, every shard with a bad tail
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/swmi.h"

extern "C" size_t fake_hip_log_size();
extern "C" const char *fake_hip_log_at(size_t);
extern "C" void fake_hip_log_clear();

#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            fprintf(stderr, "CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #cond, swmi_last_error()); \
            exit(1);                                                                                         \
        }                                                                                                    \
    } while (0)

static size_t env_size(const char *name)
{
    const char *v = getenv(name);
    CHECK(v && *v);
    return (size_t)atoll(v);
}

static std::vector<size_t> granules(size_t n, int entry)
{
    std::vector<size_t> g(swmi_host_granules_for(n, entry, nullptr, 0));
    swmi_host_granules_for(n, entry, g.data(), g.size());
    return g;
}

// tails t in [1, group) for which n = group + t has a granule in its tail group larger than every granule of a full group
static std::vector<size_t> bad_tails(size_t group, int entry)
{
    const std::vector<size_t> full = granules(group, entry);
    const size_t full_max = *std::max_element(full.begin(), full.end());
    std::vector<size_t> bad;
    for (size_t t = 1; t < group; ++t) {
        const std::vector<size_t> g = granules(group + t, entry);
        if (*std::max_element(g.begin() + full.size(), g.end()) > full_max) bad.push_back(t);
    }
    return bad;
}

// `want` tails spread over the bad ones: the smallest, the largest and evenly spaced ones between
static std::vector<size_t> spread(const std::vector<size_t> &bad, size_t want)
{
    std::vector<size_t> pick;
    if (bad.empty()) return pick;
    for (size_t k = 0; k < want; ++k) {
        const size_t t = bad[want == 1 ? 0 : k * (bad.size() - 1) / (want - 1)];
        if (pick.empty() || pick.back() != t) pick.push_back(t);
    }
    return pick;
}

static size_t stride_of(int entry) { return entry == SWMI_ENTRY_PACKED ? SWMI_PACKED_LEN : SWMI_SEQ_LEN; }

// n numbered pairs at the entry's input stride (the number in the first four bytes of seq1)
static void numbered(size_t n, size_t stride, std::vector<uint8_t> &a, std::vector<uint8_t> &b)
{
    a.assign(n * stride, 0);
    b.assign(n * stride, 0);
    for (size_t k = 0; k < n; ++k) { const uint32_t id = (uint32_t)k; memcpy(&a[k * stride], &id, 4); }
}

static int8_t g_sm[16];

// one host-batch call of `entry` on a fresh context of GPU `device`: every score, every launch, and the slot allocation
static void one_call(int entry, size_t n, int device = 0)
{
    CHECK(swmi_shutdown() == SWMI_OK);
    CHECK(swmi_init(device) == SWMI_OK);
    const size_t stride = stride_of(entry);
    std::vector<uint8_t> a, b;
    numbered(n, stride, a, b);
    std::vector<int32_t> out(n, -1);
    fake_hip_log_clear();
    const int rc = entry == SWMI_ENTRY_PAIRS  ? swmi_score_batch(a.data(), b.data(), n, g_sm, 15, out.data())
                 : entry == SWMI_ENTRY_PACKED ? swmi_score_batch_packed(a.data(), b.data(), n, g_sm, 15, out.data())
                                              : swmi_score_one_vs_many(a.data(), n, b.data(), g_sm, 15, out.data());
    CHECK(rc == SWMI_OK);
    for (size_t k = 0; k < n; ++k)
        if (out[k] != (int32_t)k) {
            fprintf(stderr, "entry %d, n %zu: score %zu reads %d\n", entry, n, k, out[k]);
            exit(1);
        }
    // one launch per granule, and the slots' input buffers sized from the largest granule of ANY group
    const std::vector<size_t> g = granules(n, entry);
    const size_t largest = *std::max_element(g.begin(), g.end());
    const std::string want = "dev" + std::to_string(device) + " malloc bytes" + std::to_string(largest * stride);
    size_t launches = 0, slot_buffers = 0;
    for (size_t k = 0; k < fake_hip_log_size(); ++k) {
        const std::string l = fake_hip_log_at(k);
        launches += l.find(entry == SWMI_ENTRY_ONE_VS_MANY ? "launch_one_vs_many" : "launch_score") != std::string::npos;
        slot_buffers += l == want;
    }
    CHECK(launches == g.size());
    CHECK(slot_buffers >= 2);           // seq1 + seq2 of at least one slot hold exactly the largest granule
    printf("  entry %d  n %zu: %zu granules, largest %zu: ok\n", entry, n, g.size(), largest);
}

int main(int argc, char **argv)
{
    CHECK(argc == 2);
    const std::string mode = argv[1];
    for (int i = 0; i < 16; ++i) g_sm[i] = int8_t(i % 5 == 0 ? 10 : -30);
    const size_t group = env_size("SWMI_TEST_SCORE_GROUP");
    CHECK(swmi_init(0) == SWMI_OK);
    const std::vector<size_t> bad = bad_tails(group, SWMI_ENTRY_PACKED);
    printf("group %zu: %zu of %zu tails give the packed entry a granule above the full group's largest\n", group, bad.size(),
           group - 1);
    CHECK(!bad.empty());                // (the sizes this driver exists for)
    // the unbalanced schedules (pairs, one-vs-many) never put a larger granule into a later group
    CHECK(bad_tails(group, SWMI_ENTRY_PAIRS).empty() && bad_tails(group, SWMI_ENTRY_ONE_VS_MANY).empty());

    if (mode == "group") {
        // the worst tail: the one whose oversized granule is the largest (smallest such tail on a tie)
        size_t worst = bad[0], worst_max = 0;
        for (size_t t : bad) {
            const std::vector<size_t> g = granules(group + t, SWMI_ENTRY_PACKED);
            const size_t m = *std::max_element(g.begin(), g.end());
            if (m > worst_max) { worst_max = m; worst = t; }
        }
        printf("worst tail %zu: a granule of %zu pairs\n", worst, worst_max);
        for (int entry : {SWMI_ENTRY_PACKED, SWMI_ENTRY_PAIRS, SWMI_ENTRY_ONE_VS_MANY}) one_call(entry, group + worst);
        for (size_t t : spread(bad, 5)) one_call(SWMI_ENTRY_PACKED, group + t);
        one_call(SWMI_ENTRY_PACKED, 2 * group + bad[0]);            // three groups, the last one bad
    } else if (mode == "small") {
        const std::vector<size_t> pick = spread(bad, 24);
        for (size_t t : pick) one_call(SWMI_ENTRY_PACKED, group + t);
        for (size_t t : spread(bad, 3))
            for (int entry : {SWMI_ENTRY_PAIRS, SWMI_ENTRY_ONE_VS_MANY}) one_call(entry, 3 * group + t);
        one_call(SWMI_ENTRY_PACKED, 3 * group);                     // no tail at all
        one_call(SWMI_ENTRY_PACKED, group - 1);                     // one group
    } else if (mode == "multi") {
        // three GPUs, equal shards of group + a bad tail each, then ragged shards whose first one has the bad tail
        CHECK(swmi_shutdown() == SWMI_OK);
        CHECK(swmi_init_all(0) == 3);
        for (size_t n : {3 * (group + bad[bad.size() / 2]), 3 * (group + bad[0]) - 2}) {      // (shards of s, s - 1, s - 1)
            size_t lo, hi;
            CHECK(swmi_shard_bounds(n, 0, 3, &lo, &hi) == SWMI_OK);
            const size_t t = hi - lo - group;
            CHECK(std::binary_search(bad.begin(), bad.end(), t));
            std::vector<uint8_t> a, b;
            numbered(n, SWMI_PACKED_LEN, a, b);
            std::vector<int32_t> out(n, -1);
            CHECK(swmi_score_batch_packed_multi(a.data(), b.data(), n, g_sm, 15, out.data()) == SWMI_OK);
            for (size_t k = 0; k < n; ++k) CHECK(out[k] == (int32_t)k);
            printf("  packed multi n %zu on 3 GPUs (shard 0: %zu pairs, tail %zu): ok\n", n, hi - lo, t);
            CHECK(swmi_shutdown() == SWMI_OK);          // the next size on fresh contexts too
            CHECK(swmi_init_all(0) == 3);
        }
    } else {
        CHECK(!"unknown mode");
    }
    CHECK(swmi_shutdown() == SWMI_OK);
    printf("host sizing fake ok\n");
    return 0;
}
