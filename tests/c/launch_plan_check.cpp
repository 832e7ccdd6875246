// Host-only check of mpich_amd/csrc/redop_launch.h, the one header it
// includes.  Built with g++ by tests/test_launch_plan.py (once more with
// -fsanitize=address,undefined, run as a program of its own).
//   launch_plan_check replay   stdin: a "facts" line, then one call per line ->
//                              its plan, or its batch steps, one line each
//                              (tests/golden/make_launch_plans.py has the formats)
//       facts unroll unroll32 block32 vblock signal_max_grid multi_lds
//       contig unit ai ao count block max_grid done done_ctr
//       multi unit ao count block max_grid k in...
//       tree unit out count max_grid is_split k in...
//       vector unit ai ao n bl st block max_grid
//       getacc unit ai ar ao count block max_grid
//       batch unit block is_split k (ai ao count)...
//   launch_plan_check props    the split's and the packing's properties over a
//                              dense sweep of units x phases x counts
#include "redop_launch.h"

#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

using namespace mpix;

static int fails = 0;

#define CHECK(cond, ...)                                                                          \
    do {                                                                                          \
        if (!(cond)) {                                                                            \
            if (++fails <= 20) {                                                                  \
                printf("FAIL %s: ", #cond);                                                       \
                printf(__VA_ARGS__);                                                              \
                printf("\n");                                                                     \
            }                                                                                     \
        }                                                                                         \
    } while (0)

static const char *form_name(Form f)
{
    switch (f) {
        case Form::PacketsAin: return "PacketsAin";
        case Form::PacketsUin: return "PacketsUin";
        case Form::Elem: return "Elem";
        case Form::Packets32: return "Packets32";
        case Form::VectorS2: return "VectorS2";
        case Form::Vector1: return "Vector1";
        case Form::Vector: return "Vector";
        case Form::Tree2x2: return "Tree2x2";
        case Form::Tree4x2: return "Tree4x2";
        case Form::Tree8x1: return "Tree8x1";
        case Form::Tree16x1: return "Tree16x1";
        case Form::TreeElem: return "TreeElem";
        case Form::TreePair32: return "TreePair32";
        case Form::GetaccAligned: return "GetaccAligned";
        case Form::GetaccUnaligned: return "GetaccUnaligned";
        case Form::GetaccElem: return "GetaccElem";
    }
    return "?";
}

static void print_plan(const LaunchPlan &p)
{
    printf("%s %d %u %u %u %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %u\n", form_name(p.form),
           (int) p.signals, p.grid, p.block, p.lds, p.pres, p.split.head, p.split.npk,
           p.split.tail_start, p.split.ntail);
}

static bool num(uint64_t &v)
{
    return scanf("%" SCNu64, &v) == 1;
}

static LaunchCfg cfg_of(uint64_t block, uint64_t max_grid)
{
    return LaunchCfg{(int) block, (int) max_grid, 0, 0, 0, 0};
}

static int replay()
{
    LaunchFacts f{};
    char kind[16];
    while (scanf("%15s", kind) == 1) {
        const std::string k = kind;
        uint64_t v[8] = {0};
        auto read = [&](int n) {
            for (int i = 0; i < n; ++i)
                if (!num(v[i]))
                    return false;
            return true;
        };
        std::vector<uintptr_t> a;
        auto read_list = [&](uint64_t n) {
            a.resize((size_t) n);
            for (auto &x : a) {
                uint64_t t;
                if (!num(t))
                    return false;
                x = (uintptr_t) t;
            }
            return true;
        };
        if (k == "facts") {
            if (!read(6))
                return 2;
            f = LaunchFacts{false, (unsigned) v[0], (unsigned) v[1], (unsigned) v[2],
                            (unsigned) v[3], (unsigned) v[4], (unsigned) v[5]};
        } else if (k == "contig") {
            if (!read(8))
                return 2;
            print_plan(plan_contig(v[1], v[2], (unsigned) v[0], v[3], cfg_of(v[4], v[5]), f,
                                   v[6] != 0, v[7] != 0));
        } else if (k == "multi") {
            if (!read(6) || !read_list(v[5]))
                return 2;
            print_plan(plan_multi(a.data(), (int) v[5], v[1], (unsigned) v[0], v[2],
                                  cfg_of(v[3], v[4]), f));
        } else if (k == "tree") {
            if (!read(6) || !read_list(v[5]))
                return 2;
            LaunchFacts g = f;
            g.is_split = v[4] != 0;
            print_plan(plan_tree(a.data(), (int) v[5], v[1], (unsigned) v[0], v[2], cfg_of(64, v[3]),
                                 g));
        } else if (k == "vector") {
            if (!read(8))
                return 2;
            print_plan(plan_vector(v[1], v[2], (unsigned) v[0], v[3], v[4], v[5],
                                   cfg_of(v[6], v[7]), f, false, false));
        } else if (k == "getacc") {
            if (!read(7))
                return 2;
            print_plan(plan_getacc(v[1], v[2], v[3], (unsigned) v[0], v[4], cfg_of(v[5], v[6])));
        } else if (k == "batch") {
            if (!read(4) || !read_list(3 * v[3]))
                return 2;
            const int n = (int) v[3];
            std::vector<uintptr_t> ai((size_t) n), ao((size_t) n);
            std::vector<uint64_t> cnt((size_t) n);
            for (int i = 0; i < n; ++i) {
                ai[(size_t) i] = a[(size_t) (3 * i)];
                ao[(size_t) i] = a[(size_t) (3 * i + 1)];
                cnt[(size_t) i] = a[(size_t) (3 * i + 2)];
            }
            LaunchFacts g = f;
            g.is_split = v[2] != 0;
            BatchPacker pack(ai.data(), ao.data(), cnt.data(), n, (unsigned) v[0], cfg_of(v[1], 0), g);
            const char *sep = "";
            for (BatchStep st; pack.next(st); sep = " ") {
                if (st.kind == BatchStep::Own)
                    printf("%sO%d", sep, st.i);
                else if (st.kind == BatchStep::Seg)
                    printf("%sS%d,%d,%u,%" PRIu64 ",%" PRIu64 ",%u,%d", sep, st.i, st.n, st.blk0,
                           st.split.head, st.split.npk, st.split.ntail, (int) st.ain);
                else
                    printf("%sF%d,%" PRIu64, sep, st.n, st.blocks);
            }
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}

// one split: head + npk E + ntail == count, head bytes < 16, ntail < E, the
// packets start on a 16-byte boundary
static void check_split(uintptr_t ao, uint64_t count, unsigned unit)
{
    const uint64_t E = 16 / unit;
    const PacketSplit s = packet_split(ao, count, unit);
    CHECK(s.head + s.npk * E + s.ntail == count && s.tail_start == s.head + s.npk * E,
          "unit %u ao %zu count %" PRIu64, unit, (size_t) ao, count);
    CHECK(s.head * unit < 16 && s.ntail < E, "unit %u ao %zu count %" PRIu64, unit, (size_t) ao,
          count);
    CHECK(s.npk == 0 || (ao + s.head * unit) % 16 == 0, "unit %u ao %zu count %" PRIu64, unit,
          (size_t) ao, count);
}

// one batch: blk0 ascending from 0 in every launch, every launch's total at
// most max_blocks, every slot's split the single call's
static void check_batch(const std::vector<uintptr_t> &ai, const std::vector<uintptr_t> &ao,
                        const std::vector<uint64_t> &cnt, unsigned unit, unsigned block,
                        const LaunchFacts &f)
{
    const LaunchCfg cfg = cfg_of(block, 0);
    BatchPacker pack(ai.data(), ao.data(), cnt.data(), (int) cnt.size(), unit, cfg, f);
    uint64_t at = 0, seen = 0;
    int slot = 0;
    for (BatchStep st; pack.next(st);) {
        if (st.kind == BatchStep::Seg) {
            const size_t i = (size_t) st.i;
            CHECK(st.n == slot && st.blk0 == at && slot < 64, "slot %d blk0 %u at %" PRIu64, st.n,
                  st.blk0, at);
            at += st.blocks;
            ++slot;
            const LaunchPlan one = plan_contig(ai[i], ao[i], unit, cnt[i], cfg, f, false, false);
            if (unit <= 16) {
                CHECK(one.form == (st.ain ? Form::PacketsAin : Form::PacketsUin) &&
                          one.split.head == st.split.head && one.split.npk == st.split.npk &&
                          one.split.ntail == st.split.ntail && one.grid == st.blocks,
                      "segment %zu unit %u", i, unit);
            } else {
                CHECK(one.form == Form::Packets32 && st.split.npk == cnt[i] && one.grid == st.blocks,
                      "segment %zu unit %u", i, unit);
            }
        } else if (st.kind == BatchStep::Flush) {
            CHECK(st.n == slot && st.blocks == at && at <= max_blocks(pack.block()) && at > 0,
                  "flush %d / %" PRIu64, st.n, st.blocks);
            at = 0;
            slot = 0;
        } else {
            CHECK(cnt[(size_t) st.i] != 0, "segment %d", st.i);
        }
        if (st.kind != BatchStep::Flush)
            ++seen;
    }
    uint64_t nonzero = 0;
    for (uint64_t c : cnt)
        nonzero += c != 0;
    CHECK(slot == 0 && seen == nonzero, "%d slots left, %" PRIu64 " of %" PRIu64, slot, seen,
          nonzero);
}

static int props()
{
    const LaunchFacts f{false, 1, 1, 64, 64, 64, 6656};
    long splits = 0, batches = 0;
    for (unsigned unit : {1u, 2u, 4u, 8u, 16u})
        for (unsigned block : {64u, 256u}) {
            const uint64_t E = 16 / unit;
            for (uintptr_t phase = 0; phase < 16; phase += unit)
                for (uint64_t count = 0; count <= 4 * E * block; ++count, ++splits) {
                    check_split(4096 + phase, count, unit);
                    // the launchers' grids cover the packets, a tile per block
                    const LaunchPlan p = plan_contig(8192 + phase, 4096 + phase, unit, count,
                                                     cfg_of(block, 0), f, false, false);
                    CHECK((uint64_t) p.grid * block >= p.split.npk && p.grid >= 1 &&
                              p.grid <= max_blocks(block),
                          "unit %u count %" PRIu64, unit, count);
                }
        }
    // batches of 64 segments over every phase pair, counts from nothing to a
    // few tiles and, every 7th, near a whole grid's
    uint64_t x = 0x5EED0003;
    auto rnd = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    for (unsigned unit : {1u, 2u, 4u, 8u, 16u, 32u})
        for (unsigned block : {64u, 1024u})
            for (int rep = 0; rep < 200; ++rep, ++batches) {
                const uint64_t E = unit <= 16 ? 16 / unit : 1;
                const uint64_t tile = (uint64_t) (unit <= 16 ? block : f.block32) * E;
                const uint64_t most = max_blocks(unit <= 16 ? block : f.block32);
                std::vector<uintptr_t> ai(64), ao(64);
                std::vector<uint64_t> cnt(64);
                for (size_t i = 0; i < 64; ++i) {
                    ai[i] = 4096 * (2 * i + 1) + rnd() % 16 / unit * unit + (rnd() % 16 == 0);
                    ao[i] = 4096 * (2 * i + 2) + rnd() % 16 / unit * unit + (rnd() % 16 == 0);
                    cnt[i] = rnd() % (4 * tile);
                    if (rnd() % 7 == 0)
                        cnt[i] = tile * (most / 2 + rnd() % most) + rnd() % tile;
                    if (rnd() % 50 == 0)
                        cnt[i] = 1ull << 45;
                }
                check_batch(ai, ao, cnt, unit, block, f);
            }
    printf("splits: %ld batches: %ld\n", splits, batches);
    return fails;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "replay")
        return replay();
    if (mode != "props")
        return 2;
    const int bad = props();
    printf("launch plan props: %s\n", bad ? "FAIL" : "ok");
    return bad ? 1 : 0;
}
