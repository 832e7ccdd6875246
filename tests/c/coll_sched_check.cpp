// coll_sched_check.cpp -- mpich_amd/csrc/coll_sched.h on its own (g++, no HIP,
// no library): tests/test_coll_sched.py builds and runs it, plain and with
// -fsanitize=address,undefined.
//
//   props   the walk (forward and reverse) against the two loop forms as they
//           stood in coll_capi.cpp, Fold, Blocks, the multipath and pipelined
//           cuts, tree_slot_source's coverage, rs_workspace's table
//   slots   stdin "P rank bit_reversed" lines -> the slot list of each
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <set>
#include <string>
#include <vector>

#include "coll_sched.h"

using namespace coll_sched;

static int failures = 0;
#define CHECK(x, ...)                                                                     \
    do {                                                                                  \
        if (!(x)) {                                                                       \
            if (++failures <= 20) {                                                       \
                fprintf(stderr, "%s:%d: %s  [", __FILE__, __LINE__, #x);                  \
                fprintf(stderr, __VA_ARGS__);                                             \
                fprintf(stderr, "]\n");                                                   \
            }                                                                             \
        }                                                                                 \
    } while (0)

struct Rec {    // one step as the old loops computed it
    int send_idx, recv_idx;
    size_t send_cnt, recv_cnt;
};

static size_t sum(const std::vector<size_t> &c, int lo, int hi)
{
    size_t t = 0;
    for (int i = lo; i < hi; ++i)
        t += c[i];
    return t;
}

// rs_recursive_halving's loop (decreasing mask), index for index
static std::vector<Rec> old_decreasing(int newrank, int pof2, const std::vector<size_t> &newcnts,
                                       int *final_idx)
{
    std::vector<Rec> out;
    int mask = pof2 >> 1, send_idx = 0, recv_idx = 0, last_idx = pof2;
    while (mask > 0) {
        int newdst = newrank ^ mask;
        size_t send_cnt, recv_cnt;
        if (newrank < newdst) {
            send_idx = recv_idx + mask;
            send_cnt = sum(newcnts, send_idx, last_idx);
            recv_cnt = sum(newcnts, recv_idx, send_idx);
        } else {
            recv_idx = send_idx + mask;
            send_cnt = sum(newcnts, send_idx, recv_idx);
            recv_cnt = sum(newcnts, recv_idx, last_idx);
        }
        out.push_back(Rec{send_idx, recv_idx, send_cnt, recv_cnt});
        send_idx = recv_idx;
        last_idx = recv_idx + mask;
        mask >>= 1;
    }
    *final_idx = recv_idx;
    return out;
}

// allreduce_rsag's loops (increasing mask, width pof2 / (2 * mask)), forward
// then the allgather's reverse, index for index
static std::vector<Rec> old_increasing(int newrank, int pof2, const std::vector<size_t> &cnts,
                                       int *final_idx, std::vector<Rec> *reverse)
{
    std::vector<Rec> out;
    int mask = 1, send_idx = 0, recv_idx = 0, last_idx = pof2;
    while (mask < pof2) {
        int newdst = newrank ^ mask;
        size_t send_cnt, recv_cnt;
        if (newrank < newdst) {
            send_idx = recv_idx + pof2 / (mask * 2);
            send_cnt = sum(cnts, send_idx, last_idx);
            recv_cnt = sum(cnts, recv_idx, send_idx);
        } else {
            recv_idx = send_idx + pof2 / (mask * 2);
            send_cnt = sum(cnts, send_idx, recv_idx);
            recv_cnt = sum(cnts, recv_idx, last_idx);
        }
        out.push_back(Rec{send_idx, recv_idx, send_cnt, recv_cnt});
        send_idx = recv_idx;
        mask <<= 1;
        if (mask < pof2)
            last_idx = recv_idx + pof2 / mask;
    }
    *final_idx = recv_idx;
    mask >>= 1;
    while (mask > 0) {
        int newdst = newrank ^ mask;
        size_t send_cnt, recv_cnt;
        if (newrank < newdst) {
            if (mask != pof2 / 2)
                last_idx = last_idx + pof2 / (mask * 2);
            recv_idx = send_idx + pof2 / (mask * 2);
            send_cnt = sum(cnts, send_idx, recv_idx);
            recv_cnt = sum(cnts, recv_idx, last_idx);
        } else {
            recv_idx = send_idx - pof2 / (mask * 2);
            send_cnt = sum(cnts, send_idx, last_idx);
            recv_cnt = sum(cnts, recv_idx, send_idx);
        }
        reverse->push_back(Rec{send_idx, recv_idx, send_cnt, recv_cnt});
        if (newrank > newdst)
            send_idx = recv_idx;
        mask >>= 1;
    }
    return out;
}

static std::vector<size_t> ragged(std::mt19937 &rng, int n)
{
    std::vector<size_t> c(n);
    for (size_t &x : c)
        x = rng() % 4 == 0 ? 0 : rng() % 2000;
    return c;
}

static bool same(const Rec &r, const Step &st, const Blocks &b)
{
    return r.send_idx == st.send_lo && r.recv_idx == st.recv_lo &&
           r.send_cnt == b.range(st.send_lo, st.send_hi) &&
           r.recv_cnt == b.range(st.recv_lo, st.recv_hi);
}

static long check_walk()
{
    std::mt19937 rng(0x5EED0C01);
    long steps = 0;
    for (int P = 1; P <= 64; ++P) {
        const int pof2 = pof2_of(P);
        const std::vector<size_t> cnts = ragged(rng, pof2);
        const Blocks b(cnts);
        // every new rank's steps, both forms: [form][newrank][step]
        std::vector<std::vector<Step>> fwd[2], rev(pof2);
        fwd[0].resize(pof2);
        fwd[1].resize(pof2);
        for (int rank = 0; rank < P; ++rank) {
            const int nr = Fold(rank, P, true).newrank;
            if (nr < 0)
                continue;
            int fin;
            std::vector<Rec> old = old_decreasing(nr, pof2, cnts, &fin);
            Window w{0, pof2};
            size_t k = 0;
            for (int mask = pof2 >> 1; mask > 0; mask >>= 1, ++k) {
                const Step st = halve(&w, nr < (nr ^ mask));
                CHECK(k < old.size() && same(old[k], st, b), "decreasing P %d nr %d step %zu", P, nr, k);
                fwd[0][nr].push_back(st);
            }
            CHECK(k == old.size() && w.lo == nr && w.hi == nr + 1 && (pof2 == 1 || fin == nr),
                  "decreasing end P %d nr %d: [%d, %d)", P, nr, w.lo, w.hi);
            std::vector<Rec> oldrev;
            old = old_increasing(nr, pof2, cnts, &fin, &oldrev);
            w = Window{0, pof2};
            k = 0;
            for (int mask = 1; mask < pof2; mask <<= 1, ++k) {
                const Step st = halve(&w, nr < (nr ^ mask));
                CHECK(k < old.size() && same(old[k], st, b), "increasing P %d nr %d step %zu", P, nr, k);
                fwd[1][nr].push_back(st);
            }
            CHECK(k == old.size() && w.lo == bitrev(nr, pof2) && w.hi == w.lo + 1 &&
                      (pof2 == 1 || fin == w.lo),
                  "increasing end P %d nr %d: [%d, %d)", P, nr, w.lo, w.hi);
            k = 0;
            for (int mask = pof2 >> 1; mask > 0; mask >>= 1, ++k) {
                const Step st = regrow(&w, nr < (nr ^ mask));
                CHECK(k < oldrev.size() && same(oldrev[k], st, b), "reverse P %d nr %d step %zu", P, nr, k);
                rev[nr].push_back(st);
            }
            CHECK(k == oldrev.size() && w.lo == 0 && w.hi == pof2, "reverse end P %d nr %d", P, nr);
            steps += (long) (fwd[0][nr].size() + fwd[1][nr].size() + rev[nr].size());
        }
        // a step's two partners mirror each other: what one sends the other receives
        for (int nr = 0; nr < pof2; ++nr) {
            size_t k = 0;
            for (int mask = pof2 >> 1; mask > 0; mask >>= 1, ++k) {
                const Step &a = fwd[0][nr][k], &p = fwd[0][nr ^ mask][k];
                const Step &ra = rev[nr][k], &rp = rev[nr ^ mask][k];
                CHECK(a.send_lo == p.recv_lo && a.send_hi == p.recv_hi && a.recv_lo == p.send_lo &&
                          a.recv_hi == p.send_hi, "mirror decreasing P %d nr %d", P, nr);
                CHECK(ra.send_lo == rp.recv_lo && ra.send_hi == rp.recv_hi, "mirror reverse P %d nr %d", P, nr);
            }
            k = 0;
            for (int mask = 1; mask < pof2; mask <<= 1, ++k) {
                const Step &a = fwd[1][nr][k], &p = fwd[1][nr ^ mask][k];
                CHECK(a.send_lo == p.recv_lo && a.send_hi == p.recv_hi && a.recv_lo == p.send_lo &&
                          a.recv_hi == p.send_hi, "mirror increasing P %d nr %d", P, nr);
            }
        }
    }
    return steps;
}

static void check_fold()
{
    std::mt19937 rng(0x5EED0C02);
    for (int P = 1; P <= 64; ++P)
        for (int odd = 0; odd < 2; ++odd) {
            const int pof2 = pof2_of(P), rem = P - pof2;
            std::set<int> seen;
            for (int r = 0; r < P; ++r) {
                const Fold f(r, P, odd);
                CHECK(f.pof2 == pof2 && f.rem == rem && f.paired == (r < 2 * rem), "fold P %d r %d", P, r);
                // the fold as the schedules wrote it
                int want = r < 2 * rem ? ((r % 2 == 1) == (odd == 1) ? r / 2 : -1) : r - rem;
                CHECK(f.newrank == want && f.newrank_of(r) == want, "newrank P %d r %d", P, r);
                if (want >= 0) {
                    CHECK(f.real(want) == r && seen.insert(want).second, "real P %d r %d", P, r);
                    CHECK(f.real(want) == (want < rem ? want * 2 + odd : want + rem), "real form");
                } else {
                    CHECK(Fold(r ^ 1, P, odd).newrank == r / 2, "partner P %d r %d", P, r);
                }
            }
            CHECK((int) seen.size() == pof2 && *seen.begin() == 0 && *seen.rbegin() == pof2 - 1,
                  "survivors P %d", P);
            if (!odd)
                continue;
            const std::vector<size_t> cnts = ragged(rng, P);
            const std::vector<size_t> nc = Fold(0, P, true).newcnts(cnts);
            for (int i = 0; i < pof2; ++i) {    // …recursive_halving.c:145-160 as it stood
                int old_i = i < rem ? i * 2 + 1 : i + rem;
                CHECK(nc[i] == (old_i < 2 * rem ? cnts[old_i] + cnts[old_i - 1] : cnts[old_i]),
                      "newcnts P %d i %d", P, i);
            }
            CHECK(Blocks(nc).total == Blocks(cnts).total, "newcnts total P %d", P);
        }
}

static void check_blocks()
{
    for (int P = 1; P <= 64; ++P)
        for (size_t count = 0; count <= (size_t) 4 * P + 3; ++count) {
            const Blocks e = Blocks::even(count, P), r = Blocks::ring(count, P);
            std::vector<size_t> ring(P, 0);     // allreduce_intra_ring.c:34-42 as it stood
            size_t total = 0;
            for (int i = 0; i < P; ++i) {
                ring[i] = (count + P - 1) / P;
                if (total + ring[i] > count) {
                    ring[i] = count - total;
                    break;
                }
                total += ring[i];
            }
            for (const Blocks *b : {&e, &r}) {
                std::vector<size_t> cs;
                for (int i = 0; i < P; ++i)
                    cs.push_back(b->cnt(i));
                CHECK(b->total == count && b->n() == P && b->disps[0] == 0 &&
                          b->disps[P] == count, "tile P %d count %zu", P, count);
                for (int i = 0; i < P; ++i)
                    CHECK(b->cnt(i) == b->disps[i + 1] - b->disps[i], "disps P %d", P);
                for (int lo = 0; lo <= P; lo += 1 + P / 7)
                    for (int hi = lo; hi <= P; ++hi)
                        CHECK(b->range(lo, hi) == sum(cs, lo, hi), "range P %d", P);
            }
            for (int i = 0; i < P; ++i) {
                CHECK(e.cnt(i) == count / P + ((size_t) i < count % P ? 1 : 0), "even P %d", P);
                CHECK(r.cnt(i) == ring[i], "ring P %d count %zu i %d", P, count, i);
            }
        }
}

static void check_cuts()
{
    for (int size = 4; size <= 64; size *= 2)
        for (int m = 1; m < size; m <<= 1) {
            const std::vector<int> A = relay_masks(m, size);
            std::multiset<int> used;
            for (int a : A) {
                CHECK(a != m && a > 0 && a < size, "relay mask");
                used.insert(a);
                used.insert(a ^ m);
            }
            CHECK((int) A.size() == size / 2 - 1 && (int) used.size() == size - 2, "relay count");
            for (int a = 1; a < size; ++a)
                CHECK((int) used.count(a) == (a == m ? 0 : 1), "relay pair size %d m %d a %d", size, m, a);
            const size_t n = A.size() + 1, D0 = n * (n - 1);
            std::vector<size_t> Ds;
            for (size_t D = D0; D < D0 + 40; ++D)
                Ds.push_back(D);
            for (size_t mib : {3, 4, 8, 9, 33, 100})    // MiB per part: 1, 1, 2, 2, 8, 8 chunks
                Ds.push_back(n * (mib << 18) + 5);
            for (size_t D : Ds) {
                const PartCut cut(D, n, 4);
                const size_t part = (cut.lo(1) - cut.lo(0)) * 4 >> 22;
                CHECK(cut.C == (part < 1 ? 1 : part > 8 ? 8 : part), "chunks D %zu", D);
                size_t at = 0;
                for (size_t j = 0; j < n; ++j) {
                    CHECK(cut.lo(j) == at && cut.lo(j + 1) - cut.lo(j) >= n - 1, "part D %zu", D);
                    for (size_t k = 0; k < cut.C; ++k) {
                        size_t off, len;
                        cut.piece(j, k, &off, &len);
                        CHECK(off == at, "piece D %zu j %zu k %zu", D, j, k);
                        at += len;
                    }
                }
                CHECK(at == D && cut.lo(n) == D, "tile D %zu", D);
            }
            CHECK(multipath_relay_bytes(1001, 4, size) == (size_t) (size / 2 - 1) * round256(4004), "relay bytes");
        }
    CHECK(multipath_shape({5, 5, 5, 5}, 4) && !multipath_shape({5, 5}, 2) &&
              !multipath_shape({5, 5, 5, 4}, 4) && !multipath_shape({1, 1, 1, 1, 1, 1}, 6), "shape");
    // the pipelined pairwise: >= 4 MiB chunks of the largest block, at most 8, none below 8 MiB
    const size_t MiB = size_t(1) << 20;
    CHECK(pipe_chunks(8 * MiB - 1) < 2 && pipe_chunks(8 * MiB) == 2 && pipe_chunks(12 * MiB) == 3 &&
              pipe_chunks(32 * MiB) == 8 && pipe_chunks(1024 * MiB) == 8 && pipe_chunks(0) == 0, "pipe chunks");
    std::mt19937 rng(0x5EED0C03);
    for (size_t nch = 2; nch <= 8; ++nch)
        for (int t = 0; t < 200; ++t) {
            const size_t n = t < 20 ? (size_t) t : rng() % (64 * MiB);
            size_t at = 0;
            for (size_t k = 0; k < nch; ++k) {
                CHECK(pipe_lo(n, k, nch) == at, "pipe chunk");
                at = pipe_lo(n, k + 1, nch);
            }
            CHECK(at == n, "pipe tile");
        }
}

static void check_slots()
{
    for (int P = 2; P <= 16; ++P)
        for (int rank = 0; rank < P; ++rank)
            for (int rev = 0; rev < 2; ++rev) {
                const Fold f(rank, P, true);
                const int nr = f.paired ? rank / 2 : f.newrank;
                std::multiset<int> got;
                int absent = 0;
                for (int sl = 0; sl < tree_slots(f.pof2, f.rem); ++sl) {
                    const int src = tree_slot_source(nr, sl, f.pof2, f.rem, rev);
                    CHECK(src >= -1 && src < P, "slot range");
                    src < 0 ? (void) ++absent : (void) got.insert(src);
                }
                CHECK((int) got.size() == P, "slot sources P %d rank %d", P, rank);
                for (int q = 0; q < P; ++q)
                    CHECK(got.count(q) == 1, "slot P %d rank %d source %d", P, rank, q);
                CHECK(absent == (f.rem ? 2 * f.pof2 - P : 0), "absent P %d", P);
                CHECK(tree_slot_source(nr, 0, f.pof2, f.rem, rev) == f.real(nr), "slot 0 is the own pair");
            }
}

static size_t old_rs_workspace(size_t total, size_t mine, size_t ext, int size, int algo)
{
    if (size == 1)
        return 0;
    const size_t whole = 2 * round256(total * ext);
    switch (algo) {     // the numbers of mpix_coll.h's MPIX_RSB_* as they stood
        case 1: return whole;
        case 6: return whole + (total == mine * (size_t) size ? (size / 2 - 1) * round256(mine * ext) : 0);
        case 2: case 4: return (size - 1) * round256(mine * ext);
        case 3: return round256(mine * ext);
        case 7: return size > 16 ? whole : 0;
        default: return 0;
    }
}

static void check_workspace()
{
    for (int size : {1, 2, 3, 4, 8, 16, 17, 32})
        for (size_t mine : {0, 1, 7, 64, 1001})
            for (size_t ext : {1, 4, 16})
                for (int algo = 0; algo <= 8; ++algo) {
                    const size_t ragged_total = mine * size + 3;
                    CHECK(rsb_workspace(mine, ext, size, algo) ==
                              old_rs_workspace(mine * size, mine, ext, size, algo), "rsb_workspace %d", algo);
                    CHECK(rs_workspace(ragged_total, mine, ext, size, algo) ==
                              old_rs_workspace(ragged_total, mine, ext, size, algo), "rs_workspace %d", algo);
                }
    CHECK(rs_choose(MPIX_RSB_AUTO, (512u << 10) - 1) == MPIX_RSB_RECURSIVE_HALVING &&
              rs_choose(MPIX_RSB_AUTO, 512u << 10) == MPIX_RSB_PAIRWISE &&
              rs_choose(MPIX_RSB_PULL, 1) == MPIX_RSB_PULL &&
              rsb_choose(MPIX_RSB_AUTO, 1 << 14, 4, 8) == MPIX_RSB_PAIRWISE, "rs_choose");
    CHECK(reduce_workspace(1000, true) == 1024 && reduce_workspace(1000, false) == 2048 &&
              round256(0) == 0 && round256(1) == 256 && round256(256) == 256, "reduce_workspace");
    CHECK(MPIX_RSB_RECURSIVE_HALVING == 1 && MPIX_RSB_PAIRWISE == 2 && MPIX_RSB_PAIRWISE_SEQUENTIAL == 3 &&
              MPIX_RSB_PAIRWISE_PIPELINED == 4 && MPIX_RSB_RECURSIVE_HALVING_MULTIPATH == 6 &&
              MPIX_RSB_RECURSIVE_HALVING_PULL == 7, "algorithm numbers");
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "props";
    if (mode == "slots") {
        int P, rank, rev;
        while (scanf("%d %d %d", &P, &rank, &rev) == 3) {
            const Fold f(rank, P, true);
            const int nr = f.paired ? rank / 2 : f.newrank;
            for (int sl = 0; sl < tree_slots(f.pof2, f.rem); ++sl)
                printf("%s%d", sl ? "," : "", tree_slot_source(nr, sl, f.pof2, f.rem, rev));
            printf("\n");
        }
        return 0;
    }
    const long steps = check_walk();
    check_fold();
    check_blocks();
    check_cuts();
    check_slots();
    check_workspace();
    printf("walk steps: %ld\n", steps);
    if (failures) {
        printf("coll_sched props: %d FAILED\n", failures);
        return 1;
    }
    printf("coll_sched props: ok\n");
    return 0;
}
