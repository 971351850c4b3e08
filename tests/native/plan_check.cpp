// CPU-only check of the host planner (vrdx_plan.h).  Two modes:
//   plan_check                              sweeps element counts under several CU counts, both value modes, both ranking
//                                           modes and every forced tile geometry: the invariants of plan_invariants.h hold of
//                                           every plan, and the sizes at which the plan changes are those of kAtomicEdges /
//                                           kBallotEdges, found again here from the functions themselves;
//                                           the segmented and the 64-bit planners (PlanSegmentedSort, PlanSort64) over the matrix of
//                                           record_trace.cpp: grids against the formulas restated here, no step of grid 0,
//                                           slots that increase, no step in a refused or empty plan;
//   plan_check describe <cus> <atomic> <n>...   one line per (n, key+value): n, 0 | 1, the plan's name (those of
//                                           vulkan_radix_sort_amd/api.py, PLAN_NAMES), its bits, hybridCap, msdCap, launches and
//                                           tile geometry -- what the Python tests hold their hand-kept numbers to.
//   plan_check describe <cus> <atomic> NAME=VALUE... <n>...   the same under planning knobs, spelled as in the environment
//                                           (VRDX_SMALL_SORT=0, VRDX_HYBRID=0, VRDX_MSD=0, VRDX_BLOCK_SUMS=0, VRDX_TILE_CONFIG=1024x8
//                                           ...; read as EnvKnobs of vrdx_api.cpp reads them), with six more fields per line:
//                                           the plan's name of a sort by the bits [8, 16), the form of the wide-value sort
//                                           (api.py, WIDE_VALUE_FORM_NAMES) and its oneWorkgroupMax, the form of the range sort
//                                           by the bits [8, 16) (api.py, RANGE_SORT_FORM_NAMES) and the form and the
//                                           launches of the range sort over [0, 32).
// Built by tests/native/Makefile; nothing of HIP is linked (vrdx_kernels.h needs one of its headers).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <string>
#include <string_view>
#include <vector>

#include "plan_invariants.h"

namespace {

// what kind of plan the host records: one workgroup | eight-bit hybrid with that capacity | MSD | four passes
struct Kind {
  bool oneWorkgroup;
  uint32_t hybridCap, msdBits, msdCap;
  bool operator==(const Kind& o) const {
    return oneWorkgroup == o.oneWorkgroup && hybridCap == o.hybridCap && msdBits == o.msdBits && msdCap == o.msdCap;
  }
};

Kind KindOf(const vrdx::SortPlan& p) { return Kind{p.oneWorkgroup, p.hybridCap, p.msdBits, p.msdBits != 0 ? p.msdCap : 0u}; }

// the same from the rules alone (no layout, no tile plan): cheap enough for every n
Kind KindByRule(const vrdx::PlanContext& c, bool keyValue, uint32_t n) {
  if (n <= vrdx::kSmallSortMaxElements) return Kind{n != 0, 0, 0, 0};  // (the empty sort records nothing)
  Kind k{false, vrdx::HybridCapacity(c, n), 0, 0};
  k.msdBits = vrdx::MsdBits(c, keyValue, n, k.hybridCap, &k.msdCap);
  if (k.msdBits == 0) k.msdCap = 0;
  return k;
}

const char* PlanName(uint32_t plan) {
  switch (plan) {
    case VRDX_HIP_PLAN_ONE_WORKGROUP: return "one-workgroup";
    case VRDX_HIP_PLAN_FOUR_PASSES: return "four-passes";
    case VRDX_HIP_PLAN_HYBRID8: return "hybrid-8";
    case VRDX_HIP_PLAN_MSD: return "msd";
    default: return "none";
  }
}

// one knob as the environment spells it; what EnvKnobs (vrdx_api.cpp) makes of it
bool SetKnob(vrdx::PlanContext& c, std::string_view knob) {
  const size_t eq = knob.find('=');
  const std::string_view name = knob.substr(0, eq), value = knob.substr(eq + 1);
  const bool off = !value.empty() && value[0] == '0';
  if (name == "VRDX_SMALL_SORT") c.smallSort = !off;
  else if (name == "VRDX_HYBRID") c.hybrid = !off;
  else if (name == "VRDX_MSD") c.msd = !off;
  else if (name == "VRDX_BLOCK_SUMS") c.blockSums = std::atoi(std::string(value).c_str()) != 0;
  else if (name == "VRDX_TILE_CONFIG") {
    c.forcedConfig = -1;
    for (int i = 0; i < vrdx::kNumTileConfigs; ++i) {
      char config[32];
      vrdx::ConfigName(vrdx::kTileConfigs[i], config, sizeof(config));
      if (value == config) c.forcedConfig = i;
    }
    return c.forcedConfig >= 0;
  } else
    return false;
  return true;
}

const char* RangeFormName(vrdx::RangeSortForm form) {
  switch (form) {
    case vrdx::RangeSortForm::kOneWorkgroup: return "one-workgroup";
    case vrdx::RangeSortForm::kWholeKey: return "whole-key";
    case vrdx::RangeSortForm::kChunked: return "chunked";
    default: return "none";
  }
}

const char* WideFormName(vrdx::WideValueForm form) {
  switch (form) {
    case vrdx::WideValueForm::kOneWorkgroup: return "one-workgroup";
    case vrdx::WideValueForm::kGather: return "gather";
    case vrdx::WideValueForm::kTwoSorts: return "two-sorts";
    default: return "none";
  }
}

int Describe(int argc, char** argv) {
  vrdx::PlanContext c;
  int first = 4;
  bool knobs = false;
  if (argc >= 5) {
    c.computeUnits = std::atoi(argv[2]);
    c.atomicRank = std::atoi(argv[3]) != 0;
    for (; first < argc && std::string_view(argv[first]).find('=') != std::string_view::npos; ++first) {
      knobs = true;
      if (!SetKnob(c, argv[first])) {
        std::fprintf(stderr, "plan_check describe: unknown knob '%s'\n", argv[first]);
        return 2;
      }
    }
    c.msd = c.msd && c.hybrid;  // (VRDX_HYBRID=0 switches the MSD plan off as well)
  }
  if (first >= argc) {
    std::fprintf(stderr, "usage: plan_check describe <cus> <atomic: 0 | 1> [NAME=VALUE]... <n>...\n");
    return 2;
  }
  for (int i = first; i < argc; ++i) {
    const uint32_t n = (uint32_t)std::strtoul(argv[i], nullptr, 10);
    for (int keyValue = 0; keyValue < 2; ++keyValue) {
      const vrdx::SortPlan p = vrdx::PlanSort(c, keyValue != 0, n, 0);  // (address 0, like vrdxHipDescribePlan)
      VrdxHipPlanInfo info = {};
      if (n != 0) vrdx::DescribePlan(p, &info);
      char config[32] = "-";
      if (p.stepCount > 1) vrdx::ConfigName(vrdx::kTileConfigs[p.configIndex], config, sizeof(config));
      std::printf("%u %d %s %u %u %u %u %s", n, keyValue, PlanName(info.plan), info.bits, p.hybridCap, p.msdBits != 0 ? p.msdCap : 0u,
                  info.launches, config);
      if (knobs) {
        const vrdx::SortPlan ranged = vrdx::PlanSortBits(c, keyValue != 0, n, 8, 16, 0);
        VrdxHipPlanInfo rangedInfo = {};
        if (ranged.stepCount != 0) vrdx::DescribePlan(ranged, &rangedInfo);  // (as vrdxHipDescribeSortBitsPlan)
        VrdxHipWideValuePlanInfo wide = {};
        const vrdx::WideValuePlan w = vrdx::PlanWideValueSort(c, n, 0);
        vrdx::DescribeWideValuePlan(c, w, &wide);
        std::printf(" %s %s %u", PlanName(rangedInfo.plan), WideFormName(w.form), wide.oneWorkgroupMax);
        const vrdx::RangeSortPlan partial = vrdx::PlanRangeSort(c, keyValue != 0, n, 8, 16, 0);  // (as vrdxHipDescribeRangeSortPlan)
        const vrdx::RangeSortPlan whole = vrdx::PlanRangeSort(c, keyValue != 0, n, 0, 32, 0);
        std::printf(" %s %s %u", RangeFormName(partial.form), RangeFormName(whole.form), whole.launches);
      }
      std::printf("\n");
    }
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && std::string_view(argv[1]) == "describe") return Describe(argc, argv);
  uint64_t cases = 0;
  int failures = 0;
  const auto fail = [&failures](const char* what, uint32_t n, uint32_t cus, int keyValue, int atomicRank, int forced) {
    if (failures < 10) std::printf("FAIL %s: n=%u cus=%u key+value=%d atomic=%d forced=%d\n", what, n, cus, keyValue, atomicRank, forced);
    ++failures;
  };

  // 1. the invariants, at every swept count and +-2 around every edge: adaptive plans at every CU count, every forced tile
  // geometry at 256 CUs (a forced geometry changes nothing that depends on the CU count but the tile plan)
  const auto check = [&](uint32_t n, bool dense) {
    for (uint32_t cus : plan_test::kCuCounts)
      for (int forced = -1; forced < vrdx::kNumTileConfigs; ++forced) {
        if (forced >= 0 && cus != 256 && !dense) continue;
        for (int keyValue = 0; keyValue < 2; ++keyValue)
          for (int atomicRank = 0; atomicRank < 2; ++atomicRank) {
            vrdx::PlanContext c;
            c.computeUnits = (int)cus;
            c.atomicRank = atomicRank != 0;
            c.forcedConfig = forced;
            const vrdx::SortPlan p = vrdx::PlanSort(c, keyValue != 0, n, 0);
            ++cases;
            if (!plan_test::PlanInvariantsHold(c, keyValue != 0, n, 0)) fail("invariants", n, cus, keyValue, atomicRank, forced);
            // the planner and the rules it is made of agree on the kind of plan, whatever the CU count
            if (forced < 0 && !(KindOf(p) == KindByRule(c, keyValue != 0, n))) fail("kind", n, cus, keyValue, atomicRank, forced);
            if (forced >= 0 && n != 0 && (p.oneWorkgroup || p.hybridCap != 0 || p.msdBits != 0)) fail("forced", n, cus, keyValue, atomicRank, forced);
          }
      }
  };
  plan_test::ForEachSweptCount(check);
  for (uint32_t edge : plan_test::kAtomicEdges)
    for (int d = -2; d <= 2; ++d) check((uint32_t)((int64_t)edge + d), true);
  for (uint32_t edge : plan_test::kBallotEdges)
    for (int d = -2; d <= 2; ++d) check((uint32_t)((int64_t)edge + d), true);

  // 2. a layout that cannot fit: one count past VRDX_MAX_ELEMENTS the reference's uint32 byte sizes wrap and the storage is
  // smaller than the keys (the entry points clamp the count, so the recorder never plans it): refused, nothing recorded
  for (int forced = -1; forced < vrdx::kNumTileConfigs; ++forced)
    for (int keyValue = 0; keyValue < 2; ++keyValue) {
      vrdx::PlanContext c{256, true};
      c.forcedConfig = forced;
      const uint32_t n = VRDX_MAX_ELEMENTS + 4u;
      const vrdx::SortPlan p = vrdx::PlanSort(c, keyValue != 0, n, 0);
      ++cases;
      if (p.fits || p.stepCount != 0 || p.launches != 0 || p.msdBits != 0 || p.blockSums || !plan_test::PlanInvariantsHold(c, keyValue != 0, n, 0))
        fail("unfittable", n, 256, keyValue, 1, forced);
    }

  // 3. the edges, found from the rules at EVERY n up to past the MSD plan's last size: the sizes behind which the kind of plan
  // changes are exactly the listed ones, keys-only and key+value, and what lies between them is what the table says
  const uint32_t scanUpTo = (1u << 26) + (1u << 20);
  for (int atomicRank = 0; atomicRank < 2; ++atomicRank)
    for (int keyValue = 0; keyValue < 2; ++keyValue) {
      const vrdx::PlanContext c{256, atomicRank != 0};
      std::vector<uint32_t> edges;
      std::vector<Kind> kinds;
      Kind last = KindByRule(c, keyValue != 0, 1);
      for (uint32_t n = 2; n <= scanUpTo; ++n) {
        const Kind k = KindByRule(c, keyValue != 0, n);
        if (k == last) continue;
        edges.push_back(n - 1);
        kinds.push_back(last);
        last = k;
      }
      kinds.push_back(last);
      cases += scanUpTo;
      const std::vector<uint32_t> wantEdges = atomicRank ? std::vector<uint32_t>(std::begin(plan_test::kAtomicEdges), std::end(plan_test::kAtomicEdges))
                                                         : std::vector<uint32_t>(std::begin(plan_test::kBallotEdges), std::end(plan_test::kBallotEdges));
      const std::vector<Kind> wantKinds =
          atomicRank ? std::vector<Kind>{{true, 0, 0, 0},      {false, 4096, 0, 0},    {false, 8192, 0, 0},    {false, 16384, 0, 0}, {false, 32768, 0, 0},
                                         {false, 0, 10, 18432}, {false, 0, 10, 36864}, {false, 0, 11, 36864}, {false, 0, 0, 0}}
                     : std::vector<Kind>{{true, 0, 0, 0}, {false, 4096, 0, 0}, {false, 8192, 0, 0}, {false, 16384, 0, 0}, {false, 0, 0, 0}};
      if (edges != wantEdges || !(kinds == wantKinds)) {
        fail("edges", 0, 256, keyValue, atomicRank, -1);
        for (size_t i = 0; i < edges.size() && i < 16; ++i)
          std::printf("  up to %u: one-workgroup %d hybridCap %u msdBits %u msdCap %u\n", edges[i], (int)kinds[i].oneWorkgroup, kinds[i].hybridCap,
                      kinds[i].msdBits, kinds[i].msdCap);
      }
      // ... and the planner says the same either side of every edge
      for (size_t i = 0; i < edges.size(); ++i)
        for (uint32_t n : {edges[i], edges[i] + 1}) {
          if (!(KindOf(vrdx::PlanSort(c, keyValue != 0, n, 0)) == kinds[i + (n - edges[i])])) fail("plan at an edge", n, 256, keyValue, atomicRank, -1);
        }
    }
  // kMsdStreamedOutputUpTo (vrdx_kernels.h) is the ten-bit plan's last size (also a static_assert of vrdx_plan.h)
  if (vrdx::kMsdStreamedOutputUpTo != plan_test::kAtomicEdges[6]) fail("kMsdStreamedOutputUpTo", vrdx::kMsdStreamedOutputUpTo, 256, 0, 1, -1);

  // 4. the segmented and the 64-bit planners over the matrix of record_trace.cpp (counts, segment counts, bit ranges, order
  // words) at every CU count, both key widths and value modes, against the rules restated here
  const uint32_t counts[] = {0u, 1u, 4096u, 4097u, 8192u, 8193u, 16384u, 16385u, (1u << 20) + 3u, VRDX_MAX_ELEMENTS};
  const uint32_t ranges[][2] = {{0, 32}, {5, 5}, {3, 20}, {9, 4}, {0, 33}};
  const uint32_t orders[] = {0u, 1u, 2u, 0x100u, 0x102u, 3u, 0x200u};
  for (uint32_t cus : plan_test::kCuCounts)
    for (uint32_t n : counts)
      for (int keyValue = 0; keyValue < 2; ++keyValue) {
        vrdx::PlanContext c;
        c.computeUnits = (int)cus;
        c.atomicRank = true;
        for (uint32_t segments : {0u, 1u, 2u * cus - 1u, 2u * cus + 1u, (1u << 20) + 1u})
          for (uint32_t keyBytes : {4u, 8u})
            for (uint32_t form = 0; form < (keyBytes == 4 ? 5u : 7u); ++form) {
              vrdx::SegmentedKey key;
              if (keyBytes == 4) key.beginBit = ranges[form][0], key.endBit = ranges[form][1];
              if (keyBytes == 8) key.order = orders[form];
              const vrdx::SegmentedPlan p = vrdx::PlanSegmentedSort(c, keyBytes, keyValue != 0, n, segments, key, 0);
              ++cases;
              const bool invalid = keyBytes == 4 ? key.beginBit > key.endBit || key.endBit > 32 : (key.order & ~0x100u) > 2;
              const bool empty = n == 0 || segments == 0 || (keyBytes == 4 && key.beginBit == key.endBit);
              bool ok = (p.refusal != nullptr) == invalid && p.stepCount <= 4;
              if (invalid || empty) ok = ok && p.stepCount == 0;
              // the caps: a mid segment holds 4097 elements and more, a large one more than the mid class takes
              const uint32_t midCap = n / 4097u, largeCap = n / (keyBytes == 8 && keyValue ? 8193u : 16385u);
              const uint32_t k = keyBytes == 4 ? 2u : 1u;
              const uint32_t want[4] = {1u, std::min(segments, 1u << 20), std::min(std::min(segments, midCap), k * cus),
                                        std::min(std::min(segments, largeCap), k * cus)};
              uint32_t seen = 0;
              for (uint32_t i = 0; i < p.stepCount && ok; ++i) {
                const vrdx::SegmentedSortStep& step = p.steps[i];
                const uint32_t what = (uint32_t)step.what;
                ok = what < 4 && step.grid != 0 && step.grid == want[what] && step.slot == what + 1 && step.name != nullptr &&
                     (i == 0 || step.slot > p.steps[i - 1].slot);
                seen |= 1u << what;
              }
              if (!invalid && !empty)  // every launch whose grid is not 0 is there, the fill and the small launch always
                for (uint32_t what = 0; what < 4; ++what) ok = ok && ((seen >> what & 1u) != 0) == (want[what] != 0);
              // the form of a plan with steps: the whole key (width 0), the range, or the order word
              if (p.stepCount != 0 && keyBytes == 4)
                ok = ok && p.rangeWidth == (form == 0 ? 0u : key.endBit - key.beginBit) && p.rangeBegin == (form == 0 ? 0u : key.beginBit);
              if (p.stepCount != 0 && keyBytes == 8) ok = ok && p.order == key.order && p.rangeWidth == 0;
              if (!ok) fail(keyBytes == 4 ? "segmented plan" : "segmented 64-bit plan", n, cus, keyValue, (int)segments, (int)form);
            }
        for (uint32_t order : orders) {
          const vrdx::Sort64Plan p = vrdx::PlanSort64(c, keyValue != 0, n, order, 0);
          ++cases;
          const bool invalid = (order & ~0x100u) > 2;
          bool ok = (p.refusal != nullptr) == invalid && p.stepCount == (invalid || n == 0 ? 0u : keyValue ? 6u : 4u);
          uint32_t sorts = 0;
          for (uint32_t i = 0; i < p.stepCount && ok; ++i) {
            ok = p.steps[i].name != nullptr && p.steps[i].slot <= 14 && (i == 0 || p.steps[i].slot > p.steps[i - 1].slot);
            sorts += p.steps[i].what == vrdx::Step64::kSortLoOther || p.steps[i].what == vrdx::Step64::kSortOtherLo;
          }
          if (p.stepCount != 0) ok = ok && sorts == 2 && p.steps[0].what == vrdx::Step64::kSplit && p.steps[0].slot == 1;
          if (!ok) fail("64-bit plan", n, cus, keyValue, 1, (int)order);
        }
      }

  std::printf("plan: %llu cases, %d failures\n", (unsigned long long)cases, failures);
  return failures != 0;
}
