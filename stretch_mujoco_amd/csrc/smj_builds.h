// THE TABLE OF STEP-KERNEL BUILDS.  The step kernel (smj_step_impl.h) is compiled 17 times (and once more as the lean twin of `step`, below), one translation unit each
// (smj_kernels_<tag>.hip; build `step` lives in smj_kernels.hip).  A translation unit, the lane emulator's Makefiles and the host
// tests select a build with SMJ_BUILD_TAG = <tag>; this header is the one place that says what the build is:
//   * its FAMILY: the capacity macros smj_model.h / smj_sat_mem.h read (SMJ_TALL*, SMJ_BIG, SMJ_NVS, SMJ_SAT*, NCH), written once
//     per family and shared by the family's twins -- a two-wavefront or per-solver twin cannot drift from its sibling;
//   * its PROPERTIES: solver(s) carried, wavefronts per env, escalation worker, default of SMJ_PROFILING.
// Symbols: smj_step_kernel_<tag>, smj_launch_step_<tag>, smj_step_kernel_<tag>_worker.  Every translation unit then describes itself
// to the host with one SmjBuildDesc (smj_step_tu.h), and smj_variants.h routes launches by those descriptors.  Plain C++: no HIP needed.
//
// A kernel's register allocation pays for every path compiled into it, so most builds carry ONE solver (smj_step_impl.h newton()): the
// Newton build keeps the family's plain name, the PGS twin has its own translation unit.  The per-stage cycle counters cost registers
// too: SMJ_PROFILING is 0 but for `prof`; `make bigprof` compiles profiling copies of some builds with -DSMJ_PROFILING=1.
#pragma once
#define SMJ_BUILDS_INCLUDED 1

#define SMJ_BUILDS(X) \
  X(step) X(pgs) X(prof) X(tall) X(mid) X(midp) X(big38) X(big38p) X(big50) X(big50p) X(big) X(sat) X(sat1) X(sat2) X(satp) X(sat32) X(sat32n)
#define SMJ_CARRIES_NEWTON 1
#define SMJ_CARRIES_PGS 2
#define SMJ_CARRIES_BOTH 3
#define SMJ_FAM_STD 0
#define SMJ_FAM_TALL 1
#define SMJ_FAM_MID 2
#define SMJ_FAM_BIG38 3
#define SMJ_FAM_BIG50 4
#define SMJ_FAM_BIG 5
#define SMJ_FAM_SAT16 6
#define SMJ_FAM_SAT32 7
//                      family         solvers             of a profiling copy | wavefronts per env, escalation worker, SMJ_PROFILING
// The standard variant without the cycle counters: they are runtime-optional but cost the kernel registers it does not have (scratch
// 144 -> 48 B per lane); its PGS twin (same stages, same arithmetic); and the same kernel WITH the counters (DevState::prof,
// SMJ_SLOT_PROF) and both solvers: what smj_step launches when the profiling slot is bound (tools/gpu_diag.py).
#define SMJ_ROW_step    SMJ_FAM_STD,   SMJ_CARRIES_NEWTON, SMJ_CARRIES_NEWTON, 1, 0, 0
#define SMJ_ROW_pgs     SMJ_FAM_STD,   SMJ_CARRIES_PGS,    SMJ_CARRIES_PGS,    1, 0, 0
#define SMJ_ROW_prof    SMJ_FAM_STD,   SMJ_CARRIES_BOTH,   SMJ_CARRIES_BOTH,   1, 0, 1
// The tall capacity variant: contact-rich scenes around the robot, and the escalation target of the standard variant and of `mid`.
// (The counters cost this variant ~0.5 KB of scratch per lane; only the standard variant has a profiling build.)
#define SMJ_ROW_tall    SMJ_FAM_TALL,  SMJ_CARRIES_BOTH,   SMJ_CARRIES_BOTH,   1, 1, 0
// The three-envs-per-CU build of the tall variant: the PRIMARY kernel of contact-rich scenes around the robot (kitchen fixtures); a
// step that needs more rows is finished by `tall`, like a step of the standard variant.  Product build: Newton only (PGS: `midp`).
#define SMJ_ROW_mid     SMJ_FAM_MID,   SMJ_CARRIES_NEWTON, SMJ_CARRIES_BOTH,   1, 0, 0
#define SMJ_ROW_midp    SMJ_FAM_MID,   SMJ_CARRIES_PGS,    SMJ_CARRIES_PGS,    1, 0, 0
// The big capacity variant (64 dof lanes): scenes with several free objects -- the reference's own scene.xml (table + 2 objects,
// models/scene.xml:21-35) and the kitchens.  big38: the robot + two free objects (scene.xml); big50: the robot + four (the kitchen of
// SURVEY.md 8(d)); both under 80 KB of LDS per env, two envs per CU, Newton only in the product (PGS: big38p / big50p).  big: the full
// 64 columns (136 KB of LDS, one env per CU), the fallback for models beyond 50 dofs and the escalation target of the other two.
#define SMJ_ROW_big38   SMJ_FAM_BIG38, SMJ_CARRIES_NEWTON, SMJ_CARRIES_BOTH,   1, 0, 0
#define SMJ_ROW_big38p  SMJ_FAM_BIG38, SMJ_CARRIES_PGS,    SMJ_CARRIES_PGS,    1, 0, 0
#define SMJ_ROW_big50   SMJ_FAM_BIG50, SMJ_CARRIES_NEWTON, SMJ_CARRIES_BOTH,   1, 0, 0
#define SMJ_ROW_big50p  SMJ_FAM_BIG50, SMJ_CARRIES_PGS,    SMJ_CARRIES_PGS,    1, 0, 0
#define SMJ_ROW_big     SMJ_FAM_BIG,   SMJ_CARRIES_BOTH,   SMJ_CARRIES_BOTH,   1, 1, 0
// The satellite build (smj_sat.h): the main tree with the standard variant's mapping (32 dof lanes / columns) plus up to 16
// satellites -- free objects, doors, drawers, knobs -- one lane each.  The kernel of kitchens: the reference's scene.xml (table + 2
// free objects), the kitchen stand-ins with free objects, exported Robocasa kitchens (robocasa_gen.py:129-239).  Larger models /
// steps: `sat32`.  Newton only, one wavefront per env, in the product AND in the profiling copy: PGS launches go to `satp` (two
// wavefronts per env) or `sat1` (one; what option pgs_two_waves = 0 selects, the comparator of `satp` in the tests); PGS stage cycles
// come from the profiling copy of `satp`.
#define SMJ_ROW_sat     SMJ_FAM_SAT16, SMJ_CARRIES_NEWTON, SMJ_CARRIES_NEWTON, 1, 0, 0
#define SMJ_ROW_sat1    SMJ_FAM_SAT16, SMJ_CARRIES_PGS,    SMJ_CARRIES_PGS,    1, 0, 0
// Newton on the 16-satellite family with TWO wavefronts per env (smj_wave.h SMJ_TWO_WAVES).  The family's 80 KB of LDS put two envs on
// a CU, so with one wavefront per env two of the CU's four SIMDs idle.  Here the env's second wavefront takes jobs off the first
// one's critical path (smj_step_impl.h helper(): a mailbox in the last 16 bytes of the LDS, two workgroup barriers per job):
//   * the satellites' forward pass (sat_forward) beside the main tree's kinematics;
//   * the moving-moving pairs of the collision stage (bounding spheres, oriented boxes, MPR / multiccd / box-box) beside the pairs
//     with the static world (smj_sat.h collision_static) -- its contacts come back in the slots NCON - 1, NCON - 2, ... and the first
//     wavefront appends them to its own (collision_convex);
//   * in every Newton iteration the satellites' 6 x 6 blocks and the search direction of the uncoupled ones (sat_hessian,
//     sat_solve_own) beside the main block's H = M + J' W J on the matrix cores;
//   * the satellites' integration (sat_integrate) beside the main tree's.
// Every job is work the first wavefront does itself in `sat`, in the same arithmetic order on the same data: same capacities (one
// family), same contact list contact for contact, the same states BIT FOR BIT (tests/test_satellites.py
// test_gpu_newton_two_wavefronts_per_env_equal_one_bit_for_bit; option newton_two_waves = 0 selects `sat`).
#define SMJ_ROW_sat2    SMJ_FAM_SAT16, SMJ_CARRIES_NEWTON, SMJ_CARRIES_NEWTON, 2, 0, 0
// PGS on the 16-satellite family with TWO wavefronts per env.  Wavefront 0 runs the step exactly as `sat1` does; during the PGS sweeps
// wavefront 1 sweeps the satellite islands (one lane each, smj_sat_pgs.h pgs_helper) BESIDE wavefront 0's sweeps of the dense system
// -- constraint islands do not see each other's rows, so the two run concurrently on two of the CU's four SIMDs, meet at one
// workgroup barrier per sweep, add their improvements and take the same decision.  Same capacities, same LDS, same results as `sat1`.
#define SMJ_ROW_satp    SMJ_FAM_SAT16, SMJ_CARRIES_PGS,    SMJ_CARRIES_PGS,    2, 0, 0
// The large satellite build, one env per CU, both solvers: models with more than 16 satellites, and the escalation target of the
// 16-satellite family -- an env whose step needs more rows / contacts / coupled satellites than that family holds is finished here
// (DevState::redo, as standard -> tall).  sat32n: its Newton kernels with TWO wavefronts per env, as `sat2` is to `sat` -- primary
// kernel and escalation worker; in the worker the second wavefront follows the first one from env to env (the env travels with the
// first job of every step).  Same states bit for bit as `sat32` (option newton_two_waves = 0 selects that one).
#define SMJ_ROW_sat32   SMJ_FAM_SAT32, SMJ_CARRIES_BOTH,   SMJ_CARRIES_BOTH,   1, 1, 0
#define SMJ_ROW_sat32n  SMJ_FAM_SAT32, SMJ_CARRIES_NEWTON, SMJ_CARRIES_NEWTON, 2, 1, 0
// The LEAN twin of `step` (smj_kernels_lean.hip): the same family and solver, with the paths a launch of the default model
// with default options can never execute compiled out (SMJ_LEAN, smj_step_impl.h mcache_bound() .. nroot()) -- same arithmetic, same
// states bit for bit, fewer registers held by dead code.  It is not a row the variant table routes to: smj_step swaps it in for `step`,
// call by call, when smj_variants.h smj_lean_eligible says every folded predicate has its folded value; hand-over target, pollers and
// sweep stay those of the standard variant.  Hence its own list: SMJ_BUILDS stays the set of builds smj_route chooses among.
// It runs TWO wavefronts per env (a lean row with waves = 2 turns on SMJ_W2_COLLISION, smj_step_impl.h): per step the second wavefront
// runs the whole collision stage -- which reads only the poses kinematics() left and writes only the contact list -- beside the first
// one's com_crb(), smooth_forces() and the contact-free head of make_constraint(); one join barrier before the contact rows.  One
// wavefront builds the list in table order, so the states are those of the one-wavefront build and of `step` BIT FOR BIT
// (tests/test_gpu_lean.py, tests/test_gpu_lean_two_waves.py).  Four envs per CU still (TreeTmp moves over dead rows of J, the mailbox into
// bytes freed in the contact list: 32 LDS granules), so two waves share a SIMD and the kernel is held to 256 registers per lane
// (amdgpu_waves_per_eu(2, 2), smj_step_tu.h).  Measured +5 % env-steps/s on the headline workload (profiles/std_two_waves_ab.txt).
#define SMJ_LEAN_BUILDS(X) X(lean)
#define SMJ_ROW_lean    SMJ_FAM_STD,   SMJ_CARRIES_NEWTON, SMJ_CARRIES_NEWTON, 2, 0, 0
// The lean build on ONE wavefront per env (smj_kernels_lean2.hip: the same unit under another tag, the whole step in series at the full
// register budget) -- what `lean` was before it took the second wavefront.  Option lean_build = 2 selects it in `lean`'s place
// (smj_variants.h smj_lean_pick): the comparator of A/B runs and of the bit-for-bit tests.  Its own list: neither SMJ_BUILDS nor
// SMJ_LEAN_BUILDS grows.
#define SMJ_LEAN_TWIN_BUILDS(X) X(lean2)
#define SMJ_ROW_lean2   SMJ_FAM_STD,   SMJ_CARRIES_NEWTON, SMJ_CARRIES_NEWTON, 1, 0, 0
#define smj_step_kernel_step smj_step_kernel   // build `step` keeps the plain symbol names
#define smj_launch_step_step smj_launch_step

#define SMJ_CAT2(a, b) a##b
#define SMJ_CAT(a, b) SMJ_CAT2(a, b)
#define SMJ_STR2(a) #a
#define SMJ_STR(a) SMJ_STR2(a)
#define SMJ_COLUMN(m, ...) m(__VA_ARGS__, ~)
#define SMJ_COL0(a, ...) a
#define SMJ_COL1(a, b, ...) b
#define SMJ_COL2(a, b, c, ...) c
#define SMJ_COL3(a, b, c, d, ...) d
#define SMJ_COL4(a, b, c, d, e, ...) e
#define SMJ_COL5(a, b, c, d, e, f, ...) f
#ifdef SMJ_BUILD_TAG   // the selected build's row (none selected -- smj_capi.hip, smj_render.hip: the standard family's capacities)
#define SMJ_BUILD_ROW SMJ_CAT(SMJ_ROW_, SMJ_BUILD_TAG)
#define SMJ_BUILD_FAM SMJ_COLUMN(SMJ_COL0, SMJ_BUILD_ROW)
#define SMJ_BUILD_WAVES SMJ_COLUMN(SMJ_COL3, SMJ_BUILD_ROW)
#define SMJ_STEP_KERNEL SMJ_CAT(smj_step_kernel_, SMJ_BUILD_TAG)
#define SMJ_LAUNCH_STEP SMJ_CAT(smj_launch_step_, SMJ_BUILD_TAG)
#if SMJ_COLUMN(SMJ_COL4, SMJ_BUILD_ROW)
#define SMJ_WORKER_KERNEL SMJ_CAT(SMJ_CAT(smj_step_kernel_, SMJ_BUILD_TAG), _worker)
#define SMJ_BUILD_WORKER_NAME SMJ_STR(SMJ_WORKER_KERNEL)
#else
#define SMJ_BUILD_WORKER_NAME nullptr
#endif
#else
#define SMJ_BUILD_FAM SMJ_FAM_STD
#endif

// ---- families: the capacity macros, once
#if SMJ_BUILD_FAM == SMJ_FAM_STD
#define SMJ_BUILD_FAMILY "std"     // 32 dofs, 80 constraint rows, 16 contacts (the defaults of smj_model.h); 40 KB of LDS per env, four envs per CU
#elif SMJ_BUILD_FAM == SMJ_FAM_TALL
#define SMJ_BUILD_FAMILY "tall"    // 32 dofs, 160 rows, 48 contacts (smj_model.h); ~80 KB of LDS, two envs per CU
#define SMJ_TALL 1
#elif SMJ_BUILD_FAM == SMJ_FAM_MID
#define SMJ_BUILD_FAMILY "mid"     // 53.3 KB of LDS per env instead of 59.8 KB -- 42 allocation granules of 1280 B, so that three envs fit a CU (163 840 B)
#define SMJ_TALL 1
#define SMJ_TALL_ROWS 128
#define SMJ_TALL_CONTACTS 44
#elif SMJ_BUILD_FAM == SMJ_FAM_BIG38
#define SMJ_BUILD_FAMILY "big38"   // 64 dof lanes, 38 columns, 160 rows, 48 contacts (smj_model.h)
#define SMJ_BIG 1
#define SMJ_NVS 38
#elif SMJ_BUILD_FAM == SMJ_FAM_BIG50
#define SMJ_BUILD_FAMILY "big50"   // 64 dof lanes, 50 columns, 160 rows, 48 contacts
#define SMJ_BIG 1
#define SMJ_NVS 50
#elif SMJ_BUILD_FAM == SMJ_FAM_BIG
#define SMJ_BUILD_FAMILY "big"     // 64 dof lanes and columns, 224 rows, 64 contacts
#define SMJ_BIG 1
#define SMJ_NVS 64
#elif SMJ_BUILD_FAM == SMJ_FAM_SAT16
#define SMJ_BUILD_FAMILY "sat16"   // 208 rows (96 of them with a dense Jacobian row: the rows that touch the main tree), 56 contacts, up to 3 satellites coupled to the robot / to each other per step: 79 KB of LDS per env, two envs per CU
#define SMJ_SAT 16
#ifndef SMJ_SAT_ROWS   // (capacity probes of tools override rows / dense rows with -D)
#define SMJ_SAT_ROWS 208
#endif
#define SMJ_SAT_CONTACTS 56
#ifndef SMJ_SAT_DENSE
#define SMJ_SAT_DENSE 96
#endif
#define SMJ_SAT_ITEMS 16
#define SMJ_SAT_EXT 3
#elif SMJ_BUILD_FAM == SMJ_FAM_SAT32
#define SMJ_BUILD_FAMILY "sat32"   // up to 32 satellites, 320 rows (256 of them dense), 64 contacts, 4 coupled satellites per step
#define SMJ_SAT 32
#define SMJ_SAT_ROWS 320
#define SMJ_SAT_CONTACTS 64
#define SMJ_SAT_DENSE 256
#define SMJ_SAT_EXT 4
#ifndef SMJ_EMUL
#define SMJ_SAT_ITEMS 40   // KNOWN DIFFERENCE, kept: the lane emulator's sat32 library has always run with smj_sat_mem.h's default of 20 row items per satellite
#endif
#define NCH 64             // a cone-Hessian block for every contact (one env per CU: the LDS is there)
#endif

// A translation unit that COMPILES the build (smj_step_tu.h; the descriptor probes of tests/routing) turns the properties into the
// macros the kernel source reads.  The lane emulator takes a build's capacities only: both solvers, one wavefront, counters in.
#ifdef SMJ_STEP_TU
#ifndef SMJ_PROFILING
#define SMJ_PROFILING SMJ_COLUMN(SMJ_COL5, SMJ_BUILD_ROW)
#endif
#if SMJ_PROFILING
#define SMJ_SOLVERS SMJ_COLUMN(SMJ_COL2, SMJ_BUILD_ROW)
#else
#define SMJ_SOLVERS SMJ_COLUMN(SMJ_COL1, SMJ_BUILD_ROW)
#endif
#if SMJ_SOLVERS == SMJ_CARRIES_NEWTON
#define SMJ_ONLY_NEWTON 1
#elif SMJ_SOLVERS == SMJ_CARRIES_PGS
#define SMJ_ONLY_PGS 1
#endif
#if SMJ_BUILD_WAVES == 2
#define SMJ_TWO_WAVES 1
#endif
#endif

// ---- what a build tells the host about itself: one constant per translation unit, every value from the macros in force there
struct DevModel;
struct DevState;
struct ihipStream_t;
struct SmjCaps { int nvp, nbp, nent, nefc, ncon, nvs, nsat; };   // nvs: dof columns of the variant's matrices (0: nvp); nsat: satellite capacity (0: a build without satellites)
// return 0, a hipError_t, or SMJ_LAUNCH_REFUSED_SOLVER (the launcher's own guard: nothing was launched).  The grid is the caller's
// (smj_step_plan.h): s.pipe_total workgroups of the primary kernel, worker_wgs of the escalation worker (s.redo_worker; else ignored)
typedef int (*SmjLaunch)(const DevModel& m, const DevState& s, int nsteps, unsigned read_flags, int worker_wgs, ihipStream_t* stream);
#define SMJ_LAUNCH_REFUSED_SOLVER (-7001)   // its own value, not a HIP error code: a genuine hipErrorInvalidValue of a launch (a bad LDS size ...) must not be mistaken for it
struct SmjBuildDesc {
  const char *tag, *family, *kernel, *worker;   // worker: the escalation worker kernel, or null
  SmjCaps caps;
  int debug_floats;
  int solvers;      // SMJ_CARRIES_*
  int waves;        // wavefronts per env
  int profiling;    // the SMJ_PROFILING of THIS object: whether the per-stage cycle counters are compiled in
  SmjLaunch launch;
  bool carries(int solver) const { return (solvers & (solver == 2 ? SMJ_CARRIES_NEWTON : SMJ_CARRIES_PGS)) != 0; }
};
#define SMJ_BUILD_DESC_INIT(launcher)                                                                                          \
  {SMJ_STR(SMJ_BUILD_TAG), SMJ_BUILD_FAMILY, SMJ_STR(SMJ_STEP_KERNEL), SMJ_BUILD_WORKER_NAME, {NVP, NBP, NENT, NEFC, NCON, NVS, NSAT}, \
   SMJ_DEBUG_FLOATS, SMJ_SOLVERS, SMJ_BUILD_WAVES, SMJ_PROFILING, launcher}
enum SmjBuildId {
#define X(tag) SMJ_B_##tag,
  SMJ_BUILDS(X)
#undef X
  SMJ_B_COUNT
};
#define X(tag) extern const SmjBuildDesc smj_build_##tag;
SMJ_BUILDS(X)
SMJ_LEAN_BUILDS(X)
SMJ_LEAN_TWIN_BUILDS(X)
#undef X
