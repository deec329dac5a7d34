// Where the Ed25519 ladder's L2 misses are served: Infinity Cache (MALL) or HBM.
//
// rocprofv3 on gfx950 has no MALL counter (the 4,012-counter list of the box,
// profiles/r04_counters_list.txt: TCC_EA0_RDREQ / _DRAM count every L2->fabric
// read, MALL hits included), so the split of the ladder's measured 17.0 KB of
// L2-miss reads per verification (FETCH_SIZE, x2 gfx950 correction) comes from
// this trace-driven model of the kernel's own access stream, CALIBRATED on that
// counter: the model's L2-miss bytes must reproduce the measured FETCH before
// its MALL-miss (= HBM) bytes are believed.
//
// Access stream (ed25519_ladder.hip, ed25519_ws.hpp): lane l's 2,432-B record
// at l * 2432; per window (65 of 2 bits over |c0|, c1 ~ 2^128), one 160-B
// entry of the lane's 12-entry joint table i(-A) + j(-R) (192-B stride,
// sector-aligned; ed25519_joint.hpp joint_index for the Booth digit pair, up to
// sign), the pair (0, 0) the shared identity entry; every 8th window one 128-B
// niels entry of each 4.2 MB fixed-base table ([k]B, [k]B', 16-bit Booth
// digits); the record's scalars once. The measured FETCH the header quotes is
// the r06 kernels' (two 8-entry tables, 3,200-B records): recalibrate on
// profiles/r10_pmc_c2.json before quoting a split for the joint table.
// Blocks of 256 lanes, dealt round-robin to the 8 XCDs; 512 blocks
// resident (2 waves per SIMD, 234 VGPRs); each XCD's L2 is 4 MB, the MALL
// 256 MB shared; 128-B lines, LRU, the MALL allocating on every L2 miss.
// Two schedules bracket reality: lockstep rounds (every resident block at the
// same window) and staggered (resident blocks at uniformly spread windows).
//
// build: g++ -O2 -std=c++17 -o /tmp/mall_sim tools/mall_sim.cpp; run: /tmp/mall_sim
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <list>
#include <random>
#include <unordered_map>
#include <vector>

struct Lru {
  size_t cap;
  std::list<uint64_t> order;  // front = most recent
  std::unordered_map<uint64_t, std::list<uint64_t>::iterator> where;
  explicit Lru(size_t c) : cap(c) { where.reserve(c * 2); }
  bool touch(uint64_t line) {  // true on hit
    auto it = where.find(line);
    if (it != where.end()) {
      order.splice(order.begin(), order, it->second);
      return true;
    }
    order.push_front(line);
    where[line] = order.begin();
    if (order.size() > cap) {
      where.erase(order.back());
      order.pop_back();
    }
    return false;
  }
};

struct Stats {
  uint64_t lanes = 0, l2_miss = 0, mall_miss = 0, accesses = 0;
};

constexpr uint64_t kLine = 128, kRec = 2432, kEntry = 192, kEntryRead = 160;
constexpr int kJointEntries = 12, kWindows = 65, kLanesPerBlock = 256, kXcd = 8, kResident = 512;
constexpr uint64_t kBTab = 1ull << 40, kBEntries = 32769, kIdentity = 1ull << 41;

int booth2(std::mt19937_64& g) {  // a 2-bit Booth digit: 0 and +-1 at 1/4 each, +-2 at 1/8 each
  const int v = (int)(g() & 7);
  return ((v + 1) >> 1) - ((v >> 2) << 2);
}
// joint table entry of the digit pair (ed25519_joint.hpp joint_select), -1 = identity
int joint_entry(int da, int dr) {
  const bool neg = da < 0 || (da == 0 && dr < 0);
  return 5 * (neg ? -da : da) + (neg ? -dr : dr) - 1;
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 4;
  for (int staggered = 0; staggered < 2; staggered++) {
    std::mt19937_64 g(7);
    std::vector<Lru> l2(kXcd, Lru(4u << 20 >> 7));
    Lru mall(256u << 20 >> 7);
    Stats st;
    const uint64_t total_blocks = (uint64_t)kResident * rounds;
    // slot state: block id, its window, its lanes' digits
    struct Slot {
      uint64_t block = 0;
      int window = 0;
      Stats acc;  // this block's counts, added to st when it completes
    };
    std::vector<Slot> slot(kResident);
    uint64_t next_block = 0;
    for (int s = 0; s < kResident; s++) {
      slot[s].block = next_block++;
      slot[s].window = staggered ? (int)(g() % kWindows) : 0;
    }
    auto access = [&](Stats& a, int xcd, uint64_t addr, uint64_t bytes) {
      for (uint64_t ln = addr / kLine; ln <= (addr + bytes - 1) / kLine; ln++) {
        a.accesses++;
        if (l2[xcd].touch(ln)) continue;
        a.l2_miss++;
        if (!mall.touch(ln)) a.mall_miss++;
      }
    };
    uint64_t done = 0;
    std::vector<int> order(kResident);
    for (int i = 0; i < kResident; i++) order[i] = i;
    while (done < total_blocks) {
      std::shuffle(order.begin(), order.end(), g);
      for (int s : order) {
        Slot& sl = slot[s];
        const int xcd = (int)(sl.block % kXcd);
        for (int t = 0; t < kLanesPerBlock; t++) {
          const uint64_t lane = sl.block * kLanesPerBlock + t;
          const uint64_t rec = lane * kRec;
          if (sl.window == 0) access(sl.acc, xcd, rec + kJointEntries * kEntry, 128);  // scalars
          const int e = joint_entry(booth2(g), booth2(g));
          access(sl.acc, xcd, e >= 0 ? rec + e * kEntry : kIdentity, kEntryRead);
          if (sl.window % 8 == 7) {
            access(sl.acc, xcd, kBTab + (g() % kBEntries) * kLine, kLine);
            access(sl.acc, xcd, kBTab + (kBEntries + g() % kBEntries) * kLine, kLine);
          }
        }
        if (++sl.window == kWindows) {
          // the first generation (cold caches; staggered: partial blocks) is not counted
          if (sl.block >= (uint64_t)kResident) {
            st.lanes += kLanesPerBlock;
            st.accesses += sl.acc.accesses;
            st.l2_miss += sl.acc.l2_miss;
            st.mall_miss += sl.acc.mall_miss;
          }
          done++;
          sl.acc = Stats();
          sl.block = next_block++;
          sl.window = 0;
        }
      }
    }
    const double per = 1.0 / (double)st.lanes;
    printf("{\"schedule\": \"%s\", \"lanes\": %llu, \"l2_miss_bytes_per_lane\": %.0f, "
           "\"hbm_bytes_per_lane\": %.0f, \"mall_hit_bytes_per_lane\": %.0f, \"accessed_bytes_per_lane\": %.0f}\n",
           staggered ? "staggered" : "lockstep", (unsigned long long)st.lanes, st.l2_miss * kLine * per,
           st.mall_miss * kLine * per, (st.l2_miss - st.mall_miss) * kLine * per, st.accesses * kLine * per);
    fflush(stdout);
  }
  return 0;
}
