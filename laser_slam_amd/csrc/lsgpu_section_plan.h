// lsgpu_section_plan.h -- what the filter sections of one lsgpu_icp_compute are made of, decided in one place.
//
// The reference section is an optional cut pass (not planned here: it changes no route), one source of normals, and up to
// three thinning stages in a fixed order -- MaxDensity, Shadow, CovarianceSampling.  Every stage reads the normals of what
// stands in front of it; whether a stage hands normals on is decided backwards from one question: does anybody behind the
// section read them.  The reading's section is its SurfaceNormalDataPointsFilter with Shadow and CovarianceSampling behind
// it.  No HIP and no handle in here, so that tests/cpp/section_plan_check.cpp can print the plan of every input on the CPU;
// ComputeRun (lsgpu_icp.hip) executes what this header decides and takes no routing decision of its own.
//
// None of the decisions changes what a module computes; they decide which grid the normals are computed on and which
// buffers travel.
#pragma once
#include <cstdint>

namespace lsgpu {
namespace section {

enum class Module { None, Sampling, SurfaceNormal };   // the reference section's normals module (ssn_knn / sn_knn)

struct Inputs {
  Module module = Module::None;
  // somebody behind the section reads the reference normals: a minimizer that is not point-to-point, the robust filter's
  // point-to-plane distance, the angle filter
  bool normals_read = false;
  bool max_density = false, ref_shadow = false, ref_cov_sampling = false;
  bool rd_normals = false, rd_shadow = false, rd_cov_sampling = false;   // the reading's SurfaceNormalDataPointsFilter and what stands behind it
  // the cloud handed over carries normals (include/lsgpu_icp.h, "carried normals"): read only where the section has no
  // normals module of its own and somebody reads the side's normals -- the reading's: the angle filter alone
  bool ref_carried = false, rd_carried = false;
  bool comm = false;          // split-scan mode
  bool side_switch = true;    // the tuning's side-stream switch
};

enum class Source {
  None,                  // no normals: the cloud as given
  Sampling,              // SamplingSurfaceNormalDataPointsFilter: its points and their normals, always together
  FinalGrid,             // SurfaceNormalDataPointsFilter on the grid the loop searches
  WholeCloud,            // ... on a grid of the whole cloud, built before the thinning
  WholeCloudDensities,   // ... with the densities MaxDensity reads
  Carried                // the cloud's own normals, beside its points like Sampling's: no module, no draws
};

enum class Stage { MaxDensity, Shadow, CovSampling };
enum class ShadowNormals { NotRun, Array, Gathered };   // beside the points, or in the grid's order through the sort's inverse

struct Plan {
  const char* refusal = nullptr;   // why the compute does not run (LSGPU_BAD_CONFIG); everything below is void then
  Source source = Source::None;
  int n_stages = 0;
  Stage stages[3] = {};
  bool emits[3] = {};              // the stage hands normals on
  ShadowNormals shadow_normals = ShadowNormals::NotRun;
  bool normals_on_final_grid = false;
  bool rd_normals = false, rd_shadow = false, rd_cov_sampling = false;
  bool rd_carried = false;         // the reading's own normals go through its section with the points
  bool side = false;               // the reading's side may run on the side stream

  bool has(Stage s) const { for (int i = 0; i < n_stages; ++i) if (stages[i] == s) return true; return false; }
  bool whole_cloud() const { return source == Source::WholeCloud || source == Source::WholeCloudDensities; }
  // the normals stand in the whole cloud's grid order and CovarianceSampling, which takes an array, is the first to read them
  bool normals_copied_out() const { return whole_cloud() && stages[0] == Stage::CovSampling; }
  // what the final grid build is handed beside the points
  bool normals_to_build() const { return n_stages ? emits[n_stages - 1] : source == Source::Sampling || source == Source::Carried; }
  bool draws_per_reference_point() const { return source == Source::Sampling || has(Stage::MaxDensity); }
};

inline Plan refuse(const char* why) { Plan p; p.refusal = why; return p; }

inline Plan plan(const Inputs& in) {
  const bool no_normals = in.module == Module::None;
  if (in.max_density && in.module != Module::SurfaceNormal)
    return refuse("compute: MaxDensityDataPointsFilter: needs the densities of SurfaceNormalDataPointsFilter with keepDensities 1 as the reference filter (sn_knn > 0)");
  if (in.rd_shadow && !in.rd_normals) return refuse("compute: ShadowDataPointsFilter on the reading needs the reading's SurfaceNormalDataPointsFilter (reading_sn_knn)");
  if (in.ref_shadow && no_normals) return refuse("compute: ShadowDataPointsFilter on the reference needs the normals of a reference filter (ssn_knn or sn_knn)");
  if (in.rd_cov_sampling && !in.rd_normals) return refuse("compute: CovarianceSamplingDataPointsFilter on the reading needs the reading's SurfaceNormalDataPointsFilter (reading_sn_knn)");
  if (in.ref_cov_sampling && no_normals) return refuse("compute: CovarianceSamplingDataPointsFilter on the reference needs the normals of a reference filter (ssn_knn or sn_knn)");
  Plan p;
  if (in.max_density) p.stages[p.n_stages++] = Stage::MaxDensity;
  if (in.ref_shadow) p.stages[p.n_stages++] = Stage::Shadow;
  if (in.ref_cov_sampling) p.stages[p.n_stages++] = Stage::CovSampling;
  // the sampling filter's normals always travel with its points; SurfaceNormalDataPointsFilter's only if somebody reads them
  const bool read = in.module == Module::Sampling || (in.module == Module::SurfaceNormal && in.normals_read);
  for (int i = p.n_stages - 1, wanted = read; i >= 0; --i, wanted = true) p.emits[i] = wanted;   // (every stage reads the one before it)
  if (in.module == Module::Sampling) p.source = Source::Sampling;
  else if (in.module == Module::SurfaceNormal && p.n_stages) p.source = in.max_density ? Source::WholeCloudDensities : Source::WholeCloud;
  else if (read) p.source = Source::FinalGrid;
  else if (no_normals && in.ref_carried && in.normals_read) p.source = Source::Carried;   // (no stage: each is refused above without a module)
  p.normals_on_final_grid = p.source == Source::FinalGrid;
  if (in.ref_shadow) p.shadow_normals = p.whole_cloud() && p.stages[0] == Stage::Shadow ? ShadowNormals::Gathered : ShadowNormals::Array;
  p.rd_normals = in.rd_normals; p.rd_shadow = in.rd_shadow; p.rd_cov_sampling = in.rd_cov_sampling;
  p.rd_carried = in.rd_carried && !in.rd_normals;   // (a module overwrites what the cloud carries)
  // The reference's grid build and the reading's side (its filter, the queries' order) do not depend on each other: the latter
  // goes to a second stream.  Both are chains of short launches that leave most of the chip idle; side by side the shorter
  // one disappears (LSGPU_NO_SIDE_STREAM: one after the other).  Not with MaxDensity: the reading's first draw is known only
  // after the thinning pass has counted the dense points.  Not with the reading's normals: they are computed on the handle's
  // grid before the reference takes it.
  p.side = in.side_switch && !in.comm && !in.rd_normals && !in.max_density;
  return p;
}

// The one decision that needs a count on the host: SurfaceNormalDataPointsFilter with CovarianceSampling alone behind it, and
// nbSample reaches what the module would be handed (`count`: the section's points behind its cut modules).  The section
// passes unchanged, so it is planned as without the module: one grid, the normals computed on it.
inline Plan settle(const Plan& p, int64_t nb_sample, int64_t count) {
  if (!p.normals_copied_out() || nb_sample < count) return p;
  Plan q = p;
  q.n_stages = 0;
  q.source = p.emits[0] ? Source::FinalGrid : Source::None;
  q.normals_on_final_grid = p.emits[0];
  return q;
}

}  // namespace section
}  // namespace lsgpu
