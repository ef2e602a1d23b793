// lsgpu_modules.h -- which modules a handle runs together: the one rule set.
//
// A handle carries eight optional modules (State), each switched on by its own setter (lsgpu_icp_set_*), all of them at once by
// lsgpu_icp_set_modules, and read from a YAML chain by the loader (lsgpu_chain_loader.cpp).  Some of them exclude each other,
// some exclude a handle configuration or the split-scan mode, two need another one.  Every such rule is ONE row of kPairs below:
// the two things that do not go together and the text each side gives when it is the one being set.  refusal() answers the one
// question all callers have -- "is this state, as it would be after my call, one the library runs?" -- for the caller that asks
// (Asker): its rules are tried in the order of its kTries list, which decides the text when two rules apply.
//
// A new module adds its flag and config to State, a Thing, its rows to kPairs and its (mine, other) entries to the kTries lists
// of the askers concerned (refusal() aborts on an entry without a row).  Value checks of a single module (robust::check,
// lsgpu_*_config_why ...) are not here: they need no second module.
//
// No HIP and no handle in this header: tests/cpp/modules_check.cpp drives it on the CPU against a recording of what the
// setters answered before it existed (tests/golden/module_rules_parent.json).
#pragma once
#include <cstdlib>
#include <string>
#include "../../include/lsgpu_icp.h"

namespace lsgpu {
namespace modules {

struct State {   // the module set of a handle, as one value
  bool robust_on = false;  lsgpu_robust_config robust{};          // RobustOutlierFilter (lsgpu_icp_set_robust_filter)
  bool normals_on = false; lsgpu_normals_config normals{};        // SurfaceNormalOutlierFilter / reading normals / orientation (lsgpu_icp_set_normals)
  bool cov_on = false;     lsgpu_covariance_config cov_cfg{};     // PointToPlaneWithCovErrorMinimizer (lsgpu_icp_set_covariance)
  bool cuts_on = false;    lsgpu_chain_cuts cuts{};               // the cut modules of the filter sections (lsgpu_icp_set_chain_cuts)
  bool md_on = false;      lsgpu_max_density_config md_cfg{};     // MaxDensityDataPointsFilter (lsgpu_icp_set_max_density)
  bool sh_on = false;      lsgpu_shadow_config sh_cfg{};          // ShadowDataPointsFilter (lsgpu_icp_set_shadow)
  bool cs_on = false;      lsgpu_cov_sampling_config cs_cfg{};    // CovarianceSamplingDataPointsFilter (lsgpu_icp_set_cov_sampling)
  bool mo_on = false;      lsgpu_motion_config mo_cfg{};          // force2D / force4DOF, BoundTransformationChecker (lsgpu_icp_set_motion)
  int dof() const { return mo_on ? mo_cfg.dof : LSGPU_MOTION_DOF_6; }
  bool bound() const { return mo_on && mo_cfg.bound != 0; }
  bool angle() const { return normals_on && normals.max_angle >= 0.f; }   // SurfaceNormalOutlierFilter itself
};

struct Facts {   // what the rules read besides the modules
  int error_minimizer = LSGPU_MINIMIZER_POINT_TO_PLANE;   // lsgpu_icp_config
  int matcher_knn = 0;                                    // lsgpu_icp_config
  bool chain = false;                                     // one of the chain thresholds of lsgpu_icp_config is set (policy::chain_fields)
  bool comm = false;                                      // the handle has a communicator (lsgpu_icp_comm_init)
};

enum Asker { kSetRobust, kSetNormalsFirst /* lsgpu_icp_set_normals in front of its value check */, kSetNormals, kSetCovariance, kSetCuts,
             kSetMaxDensity, kSetShadow, kSetCovSampling, kSetMotion, kCommInit, kLoader, kAskers };

enum Thing { kRobust, kNormals /* any lsgpu_normals_config */, kAngle, kCov, kCuts, kMaxDensity, kShadow, kCovSampling, kConstrained, kBound,
             kShadowReading, kCovSamplingReading, kNoReadingNormals, kPointToPoint, kKnn2, kChain, kComm };

inline bool holds(Thing t, const State& s, const Facts& f) {
  switch (t) {
    case kRobust: return s.robust_on;
    case kNormals: return s.normals_on;
    case kAngle: return s.angle();
    case kCov: return s.cov_on;
    case kCuts: return s.cuts_on;
    case kMaxDensity: return s.md_on;
    case kShadow: return s.sh_on;
    case kCovSampling: return s.cs_on;
    case kConstrained: return s.dof() != LSGPU_MOTION_DOF_6;
    case kBound: return s.bound();
    case kShadowReading: return s.sh_on && s.sh_cfg.reading_eps >= 0.f;
    case kCovSamplingReading: return s.cs_on && s.cs_cfg.reading_nb_sample > 0;
    case kNoReadingNormals: return !(s.normals_on && s.normals.reading_sn_knn > 0);
    case kPointToPoint: return f.error_minimizer == LSGPU_MINIMIZER_POINT_TO_POINT;
    case kKnn2: return f.matcher_knn >= 2;
    case kChain: return f.chain;
    case kComm: return f.comm;
  }
  return false;
}

// Two things that do not go together, and what is said when `a` is being set, when `b` is, and by the loader (nullptr: that side
// never asks).  "%s" stands for force2D / force4DOF.  The wording differs between the sides where it always has.
struct Pair { Thing a, b; const char* a_says; const char* b_says; const char* loader_says; };

#define LSGPU_COV "PointToPlaneWithCovErrorMinimizer: not together with "
#define LSGPU_COV_LOADER " (the covariance is implemented for knn 1 and binary distance filters)"
#define LSGPU_CON "PointToPlaneErrorMinimizer %s: not together with "
#define LSGPU_CON_LOADER "PointToPlaneErrorMinimizer: %s not together with "
#define LSGPU_CON_WHY " (the constrained steps are implemented for knn 1 and binary distance filters)"
#define LSGPU_CON_FIRST "PointToPlaneErrorMinimizer force2D / force4DOF (the constrained steps' first version takes binary distance filters)"
#define LSGPU_THINNED " (the covariance's first version does not cover a thinned reference)"
#define LSGPU_THINNED_BEHIND " (the covariance's first version does not cover a reference thinned behind the normals)"
#define LSGPU_COMM "comm_init: the split-scan mode does not run "
#define LSGPU_CUTS "MaxDist- / MinDist- / BoundingBox- / RemoveNaNDataPointsFilter in the ICP chain"
#define LSGPU_NEEDS " on the reading needs the reading's SurfaceNormalDataPointsFilter "
const Pair kPairs[] = {
    {kRobust, kComm, "RobustOutlierFilter: the split-scan mode does not run it", LSGPU_COMM "RobustOutlierFilter", nullptr},
    {kRobust, kCov, "RobustOutlierFilter: not together with PointToPlaneWithCovErrorMinimizer (its covariance takes binary weights)",
     LSGPU_COV "RobustOutlierFilter", LSGPU_COV "RobustOutlierFilter" LSGPU_COV_LOADER},
    {kRobust, kConstrained, "RobustOutlierFilter: not together with " LSGPU_CON_FIRST, LSGPU_CON "RobustOutlierFilter" LSGPU_CON_WHY,
     LSGPU_CON_LOADER "RobustOutlierFilter" LSGPU_CON_WHY},
    {kNormals, kComm, "SurfaceNormalOutlierFilter: the split-scan mode does not run it", nullptr, nullptr},
    {kAngle, kComm, nullptr, LSGPU_COMM "SurfaceNormalOutlierFilter", nullptr},
    {kAngle, kCov, "SurfaceNormalOutlierFilter: not together with PointToPlaneWithCovErrorMinimizer (its covariance pass does not apply the angle test)",
     LSGPU_COV "SurfaceNormalOutlierFilter", LSGPU_COV "SurfaceNormalOutlierFilter" LSGPU_COV_LOADER},
    {kAngle, kConstrained, "SurfaceNormalOutlierFilter: not together with " LSGPU_CON_FIRST, LSGPU_CON "SurfaceNormalOutlierFilter" LSGPU_CON_WHY,
     LSGPU_CON_LOADER "SurfaceNormalOutlierFilter" LSGPU_CON_WHY},
    {kCov, kPointToPoint, LSGPU_COV "PointToPointErrorMinimizer (the handle's minimizer)", nullptr, nullptr},
    {kCov, kKnn2, LSGPU_COV "KDTreeMatcher knn >= 2", nullptr, LSGPU_COV "KDTreeMatcher knn >= 2" LSGPU_COV_LOADER},
    {kCov, kComm, LSGPU_COV "the split-scan mode (lsgpu_icp_comm_init)", LSGPU_COMM "PointToPlaneWithCovErrorMinimizer", nullptr},
    {kCov, kMaxDensity, LSGPU_COV "MaxDensityDataPointsFilter" LSGPU_THINNED,
     "MaxDensityDataPointsFilter: not together with PointToPlaneWithCovErrorMinimizer" LSGPU_THINNED, LSGPU_COV "MaxDensityDataPointsFilter" LSGPU_THINNED},
    {kCov, kShadow, LSGPU_COV "ShadowDataPointsFilter" LSGPU_THINNED_BEHIND,
     "ShadowDataPointsFilter: not together with PointToPlaneWithCovErrorMinimizer" LSGPU_THINNED_BEHIND, LSGPU_COV "ShadowDataPointsFilter" LSGPU_THINNED_BEHIND},
    {kCov, kCovSampling, LSGPU_COV "CovarianceSamplingDataPointsFilter" LSGPU_THINNED_BEHIND,
     "CovarianceSamplingDataPointsFilter: not together with PointToPlaneWithCovErrorMinimizer" LSGPU_THINNED_BEHIND,
     LSGPU_COV "CovarianceSamplingDataPointsFilter" LSGPU_THINNED_BEHIND},
    {kCov, kConstrained, LSGPU_COV "PointToPlaneErrorMinimizer force2D / force4DOF (the covariance is that of the free 6-DOF step)",
     LSGPU_CON "PointToPlaneWithCovErrorMinimizer" LSGPU_CON_WHY, nullptr},
    {kConstrained, kPointToPoint, LSGPU_CON "PointToPointErrorMinimizer (the handle's minimizer)" LSGPU_CON_WHY, nullptr, nullptr},
    {kConstrained, kKnn2, LSGPU_CON "KDTreeMatcher knn >= 2" LSGPU_CON_WHY, nullptr, LSGPU_CON_LOADER "KDTreeMatcher knn >= 2" LSGPU_CON_WHY},
    {kConstrained, kComm, LSGPU_CON "the split-scan mode (lsgpu_icp_comm_init)" LSGPU_CON_WHY, LSGPU_COMM "PointToPlaneErrorMinimizer force2D / force4DOF", nullptr},
    {kBound, kComm, "BoundTransformationChecker: the split-scan mode (lsgpu_icp_comm_init) does not run it", LSGPU_COMM "BoundTransformationChecker", nullptr},
    {kMaxDensity, kComm, "MaxDensityDataPointsFilter: the split-scan mode (lsgpu_icp_comm_init) does not run it", LSGPU_COMM "MaxDensityDataPointsFilter", nullptr},
    {kShadow, kComm, "ShadowDataPointsFilter: the split-scan mode (lsgpu_icp_comm_init) does not run it", LSGPU_COMM "ShadowDataPointsFilter", nullptr},
    {kCovSampling, kComm, "CovarianceSamplingDataPointsFilter: the split-scan mode (lsgpu_icp_comm_init) does not run it",
     LSGPU_COMM "CovarianceSamplingDataPointsFilter", nullptr},
    {kCuts, kComm, LSGPU_CUTS ": the split-scan mode does not run them", LSGPU_COMM LSGPU_CUTS, nullptr},
    {kShadowReading, kNoReadingNormals, "ShadowDataPointsFilter" LSGPU_NEEDS "(lsgpu_icp_set_normals with reading_sn_knn) first",
     "ShadowDataPointsFilter" LSGPU_NEEDS "(reading_sn_knn): remove the module first (lsgpu_icp_set_shadow)", nullptr},
    {kCovSamplingReading, kNoReadingNormals, "CovarianceSamplingDataPointsFilter" LSGPU_NEEDS "(lsgpu_icp_set_normals with reading_sn_knn) first",
     "CovarianceSamplingDataPointsFilter" LSGPU_NEEDS "(reading_sn_knn): remove the module first (lsgpu_icp_set_cov_sampling)", nullptr},
    // (two rules about lsgpu_icp_config alone: only lsgpu_icp_comm_init can meet them)
    {kKnn2, kComm, nullptr, "comm_init: the split-scan mode runs knn 1 only (matcher_knn >= 2 is not supported there)", nullptr},
    {kChain, kComm, nullptr, "comm_init: the split-scan mode runs neither KDTreeMatcher maxDist nor Max- / Min- / MedianDistOutlierFilter", nullptr},
};
#undef LSGPU_COV
#undef LSGPU_COV_LOADER
#undef LSGPU_CON
#undef LSGPU_CON_LOADER
#undef LSGPU_CON_WHY
#undef LSGPU_CON_FIRST
#undef LSGPU_THINNED
#undef LSGPU_THINNED_BEHIND
#undef LSGPU_COMM
#undef LSGPU_CUTS
#undef LSGPU_NEEDS

// What an asker tries, in its order: (the thing it sets, what that does not go with).  kNone ends a list.
struct Try { int mine, other; };
constexpr int kNone = -1, kMaxTries = 12;
const Try kTries[kAskers][kMaxTries] = {
    /* kSetRobust */ {{kRobust, kComm}, {kRobust, kCov}, {kRobust, kConstrained}, {kNone, kNone}},
    /* kSetNormalsFirst */ {{kNoReadingNormals, kShadowReading}, {kNoReadingNormals, kCovSamplingReading}, {kNone, kNone}},
    /* kSetNormals */ {{kNormals, kComm}, {kAngle, kCov}, {kAngle, kConstrained}, {kNone, kNone}},
    /* kSetCovariance */ {{kCov, kPointToPoint}, {kCov, kKnn2}, {kCov, kRobust}, {kCov, kAngle}, {kCov, kComm}, {kCov, kMaxDensity}, {kCov, kShadow},
                          {kCov, kCovSampling}, {kCov, kConstrained}, {kNone, kNone}},
    /* kSetCuts */ {{kCuts, kComm}, {kNone, kNone}},
    /* kSetMaxDensity */ {{kMaxDensity, kComm}, {kMaxDensity, kCov}, {kNone, kNone}},
    /* kSetShadow */ {{kShadow, kComm}, {kShadow, kCov}, {kShadowReading, kNoReadingNormals}, {kNone, kNone}},
    /* kSetCovSampling */ {{kCovSampling, kComm}, {kCovSampling, kCov}, {kCovSamplingReading, kNoReadingNormals}, {kNone, kNone}},
    /* kSetMotion */ {{kConstrained, kPointToPoint}, {kConstrained, kKnn2}, {kConstrained, kRobust}, {kConstrained, kAngle}, {kConstrained, kCov},
                      {kConstrained, kComm}, {kBound, kComm}, {kNone, kNone}},
    /* kCommInit */ {{kComm, kKnn2}, {kComm, kCov}, {kComm, kMaxDensity}, {kComm, kShadow}, {kComm, kCovSampling}, {kComm, kCuts}, {kComm, kConstrained},
                     {kComm, kBound}, {kComm, kAngle}, {kComm, kRobust}, {kComm, kChain}, {kNone, kNone}},
    /* kLoader */ {{kCov, kKnn2}, {kCov, kRobust}, {kCov, kAngle}, {kCov, kMaxDensity}, {kCov, kShadow}, {kCov, kCovSampling}, {kConstrained, kKnn2},
                   {kConstrained, kRobust}, {kConstrained, kAngle}, {kNone, kNone}},
};

// Why the library does not run the state `s` (as it would be after the asker's call) on a handle with the facts `f`; empty: it does.
inline std::string refusal(const State& s, const Facts& f, Asker who) {
  for (const Try* t = kTries[who]; t->mine != kNone; ++t) {
    const Thing mine = (Thing)t->mine, other = (Thing)t->other;
    const Pair* row = nullptr;
    for (const Pair& p : kPairs)
      if ((p.a == mine && p.b == other) || (p.a == other && p.b == mine)) row = &p;
    const char* says = !row ? nullptr : who == kLoader ? row->loader_says : row->a == mine ? row->a_says : row->b_says;
    if (!says) std::abort();   // a kTries entry without its row or text: a mistake in this header, met by every run of modules_check
    if (!holds(mine, s, f) || !holds(other, s, f)) continue;
    std::string text = says;
    const size_t at = text.find("%s");
    if (at != std::string::npos) text.replace(at, 2, s.dof() == LSGPU_MOTION_DOF_3 ? "force2D" : "force4DOF");
    return text;
  }
  return std::string();
}

}  // namespace modules
}  // namespace lsgpu
