// Compat veneer, new API: TrajectoryBatch -- a device-resident batch of trajectories sharing (N, K, D), with the
// batched forms of the reference's post-solve Trajectory functions running on the MI355X through the C ABI
// (include/mtg_hip.h): evaluateRange / sampleTrajectoryInRange -> sample(), computeMinMaxMagnitude,
// computeMaxVelocityAndAcceleration, scaleSegmentTimesToMeetConstraints (src/trajectory.cpp:81-141, :190-227,
// :343-361, :385-429), and softConstraintCost -- the soft-constraint term of the time optimisers' objective
// (PolynomialOptimizationNonLinear<N>::evaluateMaximumMagnitudeAsSoftConstraint), and checkObstacleClearance -- clearance from a set
// of spheres, what a caller of the reference loops offsetTrajectory + computeMinMaxMagnitude for, checkSeparation -- the distance
// between pairs of trajectories over the time both fly, and checkKeepOutZones -- the same
// question for convex zones (boxes, prisms) given as half spaces, and checkDistanceField -- a sampled check against a voxel grid of
// distances (an ESDF), certifyDistanceField its certified form, collisionCost the cost such a grid puts on a trajectory with its
// gradient with respect to the coefficients.  Host code only: device memory goes through mtg_device_malloc / mtg_copy_*.
// The single-trajectory functions stay on the host (trajectory.h); this class is for B >> 1.
#ifndef MAV_TRAJECTORY_GENERATION_TRAJECTORY_BATCH_H_
#define MAV_TRAJECTORY_GENERATION_TRAJECTORY_BATCH_H_
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../mtg_hip.h"
#include "extremum.h"
#include "polynomial_optimization_linear.h"   // per-thread context
#include "trajectory.h"

namespace mav_trajectory_generation {

class TrajectoryBatch {
 public:
  explicit TrajectoryBatch(const std::vector<Trajectory>& trajectories) { upload(trajectories); }
  TrajectoryBatch(const TrajectoryBatch&) = delete;              // owns device memory
  TrajectoryBatch& operator=(const TrajectoryBatch&) = delete;
  ~TrajectoryBatch() { release(); }

  size_t size() const { return (size_t)B_; }
  int N() const { return N_; }
  int K() const { return K_; }
  int D() const { return D_; }
  // the device copy, for the other batched entries of the C ABI (mav_trajectory_generation_ros/feasibility_analytic.h)
  const double* deviceCoefficients() const { return coeffs_; }   // [B][K][D][N]
  const double* deviceTimes() const { return times_; }           // [B][K]

  // Per-trajectory extrema of the derivative's magnitude over `dimensions` (Trajectory::computeMinMaxMagnitude).
  bool computeMinMaxMagnitude(int derivative, const std::vector<int>& dimensions, std::vector<Extremum>* minima,
                              std::vector<Extremum>* maxima) {
    CHECK_NOTNULL(minima);
    CHECK_NOTNULL(maxima);
    if (dimensions.empty()) return false;                        // "No dimensions specified." (segment.cpp:90-93)
    uint32_t mask = 0;
    for (int dim : dimensions) {
      if (dim < 0 || dim >= D_) return false;                    // out of bounds (segment.cpp:102-107)
      mask |= 1u << dim;
    }
    if (N_ - derivative - 1 < 0) return false;                   // polynomial.cpp:70-73
    double* seg = (double*)dmalloc(sizeof(double) * 4 * B_ * K_);
    double* traj = (double*)dmalloc(sizeof(double) * 4 * B_);
    int32_t* idx = (int32_t*)dmalloc(sizeof(int32_t) * 2 * B_);
    check(mtg_minmax_magnitude(ctx(), N_, K_, D_, B_, coeffs_, times_, K_, 1, derivative, mask, seg, traj, idx));
    std::vector<double> h(4 * B_);
    std::vector<int32_t> hi(2 * B_);
    check(mtg_copy_to_host(ctx(), h.data(), traj, sizeof(double) * h.size()));
    check(mtg_copy_to_host(ctx(), hi.data(), idx, sizeof(int32_t) * hi.size()));
    mtg_device_free(ctx(), seg);
    mtg_device_free(ctx(), traj);
    mtg_device_free(ctx(), idx);
    minima->resize(B_);
    maxima->resize(B_);
    for (int64_t b = 0; b < B_; ++b) {
      (*minima)[b] = Extremum(h[4 * b + 0], h[4 * b + 1], hi[2 * b + 0]);
      (*maxima)[b] = Extremum(h[4 * b + 2], h[4 * b + 3], hi[2 * b + 1]);
    }
    return true;
  }

  // Per-trajectory SIGNED extrema of every axis (Polynomial::computeMinMax over all segments, mtg_minmax_axes): minima and
  // maxima have size() * D() entries, axis fastest; Extremum = (segment-local time, value, segment index).
  bool computeAxisMinMax(int derivative, std::vector<Extremum>* minima, std::vector<Extremum>* maxima) {
    CHECK_NOTNULL(minima);
    CHECK_NOTNULL(maxima);
    if (derivative < 0 || derivative > 4 || N_ - derivative - 1 < 0 || D_ > 8) return false;   // polynomial.cpp:70-73
    const size_t rows = (size_t)B_ * D_;
    double* seg = (double*)dmalloc(sizeof(double) * 4 * rows * K_);
    double* traj = (double*)dmalloc(sizeof(double) * 4 * rows);
    int32_t* idx = (int32_t*)dmalloc(sizeof(int32_t) * 2 * rows);
    check(mtg_minmax_axes(ctx(), N_, K_, D_, B_, coeffs_, times_, K_, 1, derivative, 1, seg, traj, idx));
    std::vector<double> h(4 * rows);
    std::vector<int32_t> hi(2 * rows);
    check(mtg_copy_to_host(ctx(), h.data(), traj, sizeof(double) * h.size()));
    check(mtg_copy_to_host(ctx(), hi.data(), idx, sizeof(int32_t) * hi.size()));
    mtg_device_free(ctx(), seg);
    mtg_device_free(ctx(), traj);
    mtg_device_free(ctx(), idx);
    minima->resize(rows);
    maxima->resize(rows);
    for (size_t r = 0; r < rows; ++r) {
      (*minima)[r] = Extremum(h[4 * r + 0], h[4 * r + 1], hi[2 * r + 0]);
      (*maxima)[r] = Extremum(h[4 * r + 2], h[4 * r + 3], hi[2 * r + 1]);
    }
    return true;
  }

  // Axis-aligned bounding box of every trajectory's position: lo and hi have size() * D() entries, axis fastest.
  bool boundingBoxes(std::vector<double>* lo, std::vector<double>* hi) {
    CHECK_NOTNULL(lo);
    CHECK_NOTNULL(hi);
    std::vector<Extremum> mn, mx;
    if (!computeAxisMinMax(derivative_order::POSITION, &mn, &mx)) return false;
    lo->resize(mn.size());
    hi->resize(mx.size());
    for (size_t r = 0; r < mn.size(); ++r) {
      (*lo)[r] = mn[r].value;
      (*hi)[r] = mx[r].value;
    }
    return true;
  }

  bool computeMaxVelocityAndAcceleration(std::vector<double>* v_max, std::vector<double>* a_max) {
    CHECK_NOTNULL(v_max);
    CHECK_NOTNULL(a_max);
    std::vector<int> dimensions(D_);
    for (int d = 0; d < D_; ++d) dimensions[d] = d;
    std::vector<Extremum> mn, mx;
    bool ok = computeMinMaxMagnitude(derivative_order::VELOCITY, dimensions, &mn, &mx);
    v_max->resize(B_);
    for (int64_t b = 0; b < B_ && ok; ++b) (*v_max)[b] = mx[b].value;
    ok = ok && computeMinMaxMagnitude(derivative_order::ACCELERATION, dimensions, &mn, &mx);
    a_max->resize(B_);
    for (int64_t b = 0; b < B_ && ok; ++b) (*a_max)[b] = mx[b].value;
    return ok;
  }

  // The soft-constraint cost of every trajectory (the third term of PolynomialOptimizationNonLinear<N>::
  // getTotalCostWithSoftConstraints): sum over `constraints` = (derivative, maximum allowed magnitude) pairs, in their order, of
  // min(maximum_cost, exp(weight * (max ||p^(derivative)|| / value - 1))).  maxima (optional): [size()][constraints.size()].
  // false: more than MTG_MAX_MAGNITUDE_CONSTRAINTS constraints, a derivative outside 1 .. N/2 - 1, a value <= 0 or D > 4.
  bool softConstraintCost(const std::vector<std::pair<int, double>>& constraints, double weight, std::vector<double>* cost,
                          std::vector<double>* maxima = nullptr, double maximum_cost = 1.0e12) {
    CHECK_NOTNULL(cost);
    if (constraints.size() > MTG_MAX_MAGNITUDE_CONSTRAINTS || D_ > 4) return false;
    mtg_time_objective_params params;
    mtg_time_objective_params_init(&params);
    params.soft_constraint_weight = weight;
    params.maximum_cost = maximum_cost;
    params.n_constraints = (int32_t)constraints.size();
    for (size_t q = 0; q < constraints.size(); ++q) {
      if (constraints[q].first < 1 || constraints[q].first > N_ / 2 - 1 || !(constraints[q].second > 0.0)) return false;
      params.derivative[q] = constraints[q].first;
      params.value[q] = constraints[q].second;
    }
    const size_t n = constraints.size();
    double* d_cost = (double*)dmalloc(sizeof(double) * B_);
    double* d_max = n ? (double*)dmalloc(sizeof(double) * B_ * n) : nullptr;
    check(mtg_magnitude_soft_cost(ctx(), N_, K_, D_, B_, coeffs_, times_, K_, 1, &params, d_cost, d_max, nullptr));
    cost->resize(B_);
    check(mtg_copy_to_host(ctx(), cost->data(), d_cost, sizeof(double) * B_));
    if (maxima) {
      maxima->resize(B_ * n);
      if (n) check(mtg_copy_to_host(ctx(), maxima->data(), d_max, sizeof(double) * B_ * n));
    }
    mtg_device_free(ctx(), d_cost);
    if (d_max) mtg_device_free(ctx(), d_max);
    return true;
  }

  // Clearance of every trajectory from a set of spheres (mtg_check_obstacle_clearance): obstacles = M x (cx, cy, cz, r), shared by
  // all trajectories; inflation = the vehicle's radius.  feasible[b]: min over [0, T] of ||p(t) - c|| - r - inflation > 0 for every
  // sphere and segment; first_segment / first_obstacle: the first failing segment and its smallest failing sphere (-1: none);
  // clearance[b]: the minimum itself (NaN wins).  The outputs are optional.  false: no or more than 4096 spheres, D not 3 or 4, more
  // than 2^19 - 1 segments, a negative or non-finite inflation.  Returns true when the check ran, whatever the verdicts.
  bool checkObstacleClearance(const std::vector<double>& obstacles, double inflation, std::vector<char>* feasible,
                              std::vector<int>* first_segment = nullptr, std::vector<int>* first_obstacle = nullptr,
                              std::vector<double>* clearance = nullptr) {
    const size_t m = obstacles.size() / 4;
    if (obstacles.size() % 4 != 0 || m < 1 || m > 4096 || !(D_ == 3 || D_ == 4) || K_ >= (1 << 19)) return false;
    if (!(inflation >= 0.0) || inflation > 1.7976931348623157e308) return false;
    double* d_obs = (double*)dmalloc(sizeof(double) * obstacles.size());
    check(mtg_copy_to_device(ctx(), d_obs, obstacles.data(), sizeof(double) * obstacles.size()));
    int32_t* d_int = (int32_t*)dmalloc(sizeof(int32_t) * 3 * B_);
    double* d_clear = (double*)dmalloc(sizeof(double) * B_);
    check(mtg_check_obstacle_clearance(ctx(), N_, K_, D_, B_, coeffs_, times_, K_, 1, d_obs, (int32_t)m, 0, inflation, d_int, d_int + B_,
                                       d_int + 2 * B_, nullptr, nullptr, nullptr, d_clear));
    std::vector<int32_t> h(3 * B_);
    check(mtg_copy_to_host(ctx(), h.data(), d_int, sizeof(int32_t) * h.size()));
    if (clearance) {
      clearance->resize(B_);
      check(mtg_copy_to_host(ctx(), clearance->data(), d_clear, sizeof(double) * B_));
    }
    mtg_device_free(ctx(), d_obs);
    mtg_device_free(ctx(), d_int);
    mtg_device_free(ctx(), d_clear);
    if (feasible) feasible->resize(B_);
    if (first_segment) first_segment->resize(B_);
    if (first_obstacle) first_obstacle->resize(B_);
    for (int64_t b = 0; b < B_; ++b) {
      if (feasible) (*feasible)[b] = (char)(h[b] != 0);
      if (first_segment) (*first_segment)[b] = h[B_ + b];
      if (first_obstacle) (*first_obstacle)[b] = h[2 * B_ + b];
    }
    return true;
  }

  // Separation of trajectories of this batch (side A) from trajectories of `other` (side B, possibly this batch itself)
  // (mtg_check_trajectory_separation): pairs = P x (index into this batch, index into other); start_a / start_b = the global time at
  // which each trajectory starts (empty: 0); min_separation = the required centre-to-centre distance.  feasible[p]:
  // ||pA(t) - pB(t)|| - min_separation > 0 at every instant both fly (a pair that never flies at the same time is feasible with
  // separation +inf); first_segment_a / _b: the earliest failing piece (-1: none); separation[p]: the minimum itself (NaN wins);
  // closest_time[p]: its GLOBAL time (NaN: none).  A pair with an index out of range, a negative or non-finite segment time or a
  // non-finite start is infeasible with NaN separation.  The outputs are optional.  false: the two batches differ in N or D, D not 3
  // or 4, more than 1024 segments on a side, pairs.size() odd, a start vector of the wrong size, a negative or non-finite
  // min_separation.  Returns true when the check ran, whatever the verdicts.
  bool checkSeparation(const TrajectoryBatch& other, const std::vector<int32_t>& pairs, double min_separation,
                       const std::vector<double>& start_a, const std::vector<double>& start_b, std::vector<char>* feasible,
                       std::vector<int>* first_segment_a = nullptr, std::vector<int>* first_segment_b = nullptr,
                       std::vector<double>* separation = nullptr, std::vector<double>* closest_time = nullptr) {
    const int64_t P = (int64_t)(pairs.size() / 2);
    if (pairs.size() % 2 != 0 || other.N_ != N_ || other.D_ != D_ || !(D_ == 3 || D_ == 4) || K_ > 1024 || other.K_ > 1024) return false;
    if ((!start_a.empty() && (int64_t)start_a.size() != B_) || (!start_b.empty() && (int64_t)start_b.size() != other.B_)) return false;
    if (!(min_separation >= 0.0) || min_separation > 1.7976931348623157e308 || P > 0x7fffffffll / K_) return false;
    if (feasible) feasible->resize(P);
    if (first_segment_a) first_segment_a->resize(P);
    if (first_segment_b) first_segment_b->resize(P);
    if (separation) separation->resize(P);
    if (closest_time) closest_time->resize(P);
    if (P == 0) return true;
    auto to_device = [&](const void* src, size_t bytes) {
      void* d = dmalloc(bytes);
      check(mtg_copy_to_device(ctx(), d, src, bytes));
      return d;
    };
    double* d_sa = start_a.empty() ? nullptr : (double*)to_device(start_a.data(), sizeof(double) * start_a.size());
    double* d_sb = start_b.empty() ? nullptr : (double*)to_device(start_b.data(), sizeof(double) * start_b.size());
    int32_t* d_pairs = (int32_t*)to_device(pairs.data(), sizeof(int32_t) * pairs.size());
    int32_t* d_int = (int32_t*)dmalloc(sizeof(int32_t) * (5 + 2 * K_) * P);      // feasible, first a, first b, closest a, closest b, 2 x [P][K]
    double* d_dbl = (double*)dmalloc(sizeof(double) * (2 + 2 * K_) * P);         // separation, closest time, 2 x [P][K]
    check(mtg_check_trajectory_separation(ctx(), N_, D_, K_, B_, coeffs_, times_, K_, 1, d_sa, other.K_, other.B_, other.coeffs_, other.times_,
                                          other.K_, 1, d_sb, P, d_pairs, min_separation, d_int, d_int + P, d_int + 2 * P, d_dbl, d_dbl + P,
                                          d_int + 3 * P, d_int + 4 * P, d_dbl + 2 * P, d_dbl + (2 + K_) * P, d_int + 5 * P,
                                          d_int + (5 + K_) * P));
    std::vector<int32_t> h(3 * P);
    std::vector<double> hd(2 * P);
    check(mtg_copy_to_host(ctx(), h.data(), d_int, sizeof(int32_t) * h.size()));
    check(mtg_copy_to_host(ctx(), hd.data(), d_dbl, sizeof(double) * hd.size()));
    if (d_sa) mtg_device_free(ctx(), d_sa);
    if (d_sb) mtg_device_free(ctx(), d_sb);
    mtg_device_free(ctx(), d_pairs);
    mtg_device_free(ctx(), d_int);
    mtg_device_free(ctx(), d_dbl);
    for (int64_t p = 0; p < P; ++p) {
      if (feasible) (*feasible)[p] = (char)(h[p] != 0);
      if (first_segment_a) (*first_segment_a)[p] = h[P + p];
      if (first_segment_b) (*first_segment_b)[p] = h[2 * P + p];
      if (separation) (*separation)[p] = hd[p];
      if (closest_time) (*closest_time)[p] = hd[P + p];
    }
    return true;
  }

  // Whether every trajectory stays OUTSIDE a set of convex keep-out zones (mtg_check_keep_out_zones): zones = M x n_planes x (nx, ny,
  // nz, offset), unit normals pointing into the zone, offset = point . normal (the six planes of HalfPlane::createBoundingBox are a
  // box), shared by all trajectories; inflation = the vehicle's radius.  feasible[b]: min over [0, T] of max_j (offset_j - n_j . p(t))
  // - inflation > 0 for every zone and segment; first_segment / first_zone: the first failing segment and its smallest failing zone
  // (-1: none); clearance[b]: the minimum itself (NaN wins).  The outputs are optional.  false: n_planes not in 1 .. 8, no or more
  // than 4096 zones, D not 3 or 4, more than 2^19 - 1 segments, a negative or non-finite inflation.  Returns true when the check ran.
  bool checkKeepOutZones(const std::vector<double>& zones, int n_planes, double inflation, std::vector<char>* feasible,
                         std::vector<int>* first_segment = nullptr, std::vector<int>* first_zone = nullptr,
                         std::vector<double>* clearance = nullptr) {
    if (n_planes < 1 || n_planes > 8 || zones.size() % (4 * (size_t)n_planes) != 0) return false;
    const size_t m = zones.size() / (4 * (size_t)n_planes);
    if (m < 1 || m > 4096 || !(D_ == 3 || D_ == 4) || K_ >= (1 << 19)) return false;
    if (!(inflation >= 0.0) || inflation > 1.7976931348623157e308) return false;
    double* d_zones = (double*)dmalloc(sizeof(double) * zones.size());
    check(mtg_copy_to_device(ctx(), d_zones, zones.data(), sizeof(double) * zones.size()));
    int32_t* d_int = (int32_t*)dmalloc(sizeof(int32_t) * 3 * B_);
    double* d_clear = (double*)dmalloc(sizeof(double) * B_);
    check(mtg_check_keep_out_zones(ctx(), N_, K_, D_, B_, coeffs_, times_, K_, 1, d_zones, (int32_t)m, n_planes, 0, inflation, d_int,
                                   d_int + B_, d_int + 2 * B_, nullptr, nullptr, nullptr, d_clear));
    std::vector<int32_t> h(3 * B_);
    check(mtg_copy_to_host(ctx(), h.data(), d_int, sizeof(int32_t) * h.size()));
    if (clearance) {
      clearance->resize(B_);
      check(mtg_copy_to_host(ctx(), clearance->data(), d_clear, sizeof(double) * B_));
    }
    mtg_device_free(ctx(), d_zones);
    mtg_device_free(ctx(), d_int);
    mtg_device_free(ctx(), d_clear);
    if (feasible) feasible->resize(B_);
    if (first_segment) first_segment->resize(B_);
    if (first_zone) first_zone->resize(B_);
    for (int64_t b = 0; b < B_; ++b) {
      if (feasible) (*feasible)[b] = (char)(h[b] != 0);
      if (first_segment) (*first_segment)[b] = h[B_ + b];
      if (first_zone) (*first_zone)[b] = h[2 * B_ + b];
    }
    return true;
  }

  // Whether every trajectory is collision-free at every SAMPLE in a voxel grid of distances (mtg_check_distance_field; between
  // samples nothing is certified): field.distances is a DEVICE pointer (DeviceDistanceField below uploads a host grid once), the rest
  // of the struct is read on the host.  Every segment is sampled at local times 0, i dt < T and T; feasible[b]: distance(p(t)) -
  // inflation > 0 at every sample of every segment, and no segment with more than max_samples samples; first_segment: the first
  // failing segment (-1: none); clearance[b]: the minimum itself (NaN wins).  The outputs are optional.  false: arguments the check
  // refuses (include/mtg_hip.h).  Returns true when the check ran, whatever the verdicts.
  bool checkDistanceField(const mtg_distance_field& field, double dt, double inflation, std::vector<char>* feasible,
                          std::vector<int>* first_segment = nullptr, std::vector<double>* clearance = nullptr, int max_samples = 4096) {
    int32_t* d_int = (int32_t*)dmalloc(sizeof(int32_t) * 2 * B_);
    double* d_clear = (double*)dmalloc(sizeof(double) * B_);
    const int rc = mtg_check_distance_field(ctx(), N_, K_, D_, B_, coeffs_, times_, K_, 1, &field, dt, max_samples, inflation, d_int,
                                            d_int + B_, nullptr, nullptr, nullptr, nullptr, d_clear);
    if (rc == MTG_OK) {
      std::vector<int32_t> h(2 * B_);
      check(mtg_copy_to_host(ctx(), h.data(), d_int, sizeof(int32_t) * h.size()));
      if (clearance) {
        clearance->resize(B_);
        check(mtg_copy_to_host(ctx(), clearance->data(), d_clear, sizeof(double) * B_));
      }
      if (feasible) feasible->resize(B_);
      if (first_segment) first_segment->resize(B_);
      for (int64_t b = 0; b < B_; ++b) {
        if (feasible) (*feasible)[b] = (char)(h[b] != 0);
        if (first_segment) (*first_segment)[b] = h[B_ + b];
      }
    }
    mtg_device_free(ctx(), d_int);
    mtg_device_free(ctx(), d_clear);
    if (rc != MTG_OK && rc != MTG_ERR_INVALID_ARGUMENT) check(rc);
    return rc == MTG_OK;
  }

  // The CERTIFIED form of checkDistanceField (mtg_certify_distance_field): a verdict for every instant of every segment.
  // field.distances is a DEVICE pointer (DeviceDistanceField), the field trilinear, lipschitz a Lipschitz constant of its
  // interpolant (mtg_distance_field_lipschitz_host on the host grid).  result[b]: MTG_FIELD_COLLIDES / FREE / UNDECIDED_DEPTH /
  // UNDECIDED_BUDGET of the first segment that is not FREE (else FREE); first_segment: that segment (-1: none); lower_bound[b]: a
  // guaranteed lower bound of the minimum of distance - inflation over the whole trajectory; sampled_clearance[b]: the lowest
  // evaluated sample, an upper bound of it.  The outputs are optional.  false: arguments the check refuses (include/mtg_hip.h).
  // Returns true when the check ran, whatever the verdicts.
  bool certifyDistanceField(const mtg_distance_field& field, double lipschitz, double inflation, std::vector<int>* result,
                            std::vector<int>* first_segment = nullptr, std::vector<double>* lower_bound = nullptr,
                            std::vector<double>* sampled_clearance = nullptr, int min_depth = 4, int max_depth = 16,
                            int max_frontier = 1024) {
    int32_t* d_int = (int32_t*)dmalloc(sizeof(int32_t) * 2 * B_);
    double* d_bound = (double*)dmalloc(sizeof(double) * 2 * B_);
    const int rc = mtg_certify_distance_field(ctx(), N_, K_, D_, B_, coeffs_, times_, K_, 1, &field, lipschitz, min_depth, max_depth,
                                              max_frontier, inflation, d_int, d_int + B_, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                              nullptr, d_bound, d_bound + B_);
    if (rc == MTG_OK) {
      std::vector<int32_t> h(2 * B_);
      check(mtg_copy_to_host(ctx(), h.data(), d_int, sizeof(int32_t) * h.size()));
      if (lower_bound) {
        lower_bound->resize(B_);
        check(mtg_copy_to_host(ctx(), lower_bound->data(), d_bound, sizeof(double) * B_));
      }
      if (sampled_clearance) {
        sampled_clearance->resize(B_);
        check(mtg_copy_to_host(ctx(), sampled_clearance->data(), d_bound + B_, sizeof(double) * B_));
      }
      if (result) result->assign(h.begin(), h.begin() + B_);
      if (first_segment) first_segment->assign(h.begin() + B_, h.end());
    }
    mtg_device_free(ctx(), d_int);
    mtg_device_free(ctx(), d_bound);
    if (rc != MTG_OK && rc != MTG_ERR_INVALID_ARGUMENT) check(rc);
    return rc == MTG_OK;
  }

  // The distance-field collision COST of every trajectory and its gradient with respect to the polynomial coefficients
  // (mtg_collision_cost): the map term of a CHOMP-style objective, sum over the samples (local times 0, i dt < T and T, trapezoid
  // weights w) of w c(distance(p(t)) - inflation) sqrt(|v(t)|^2 + speed_epsilon^2), c the CHOMP potential that vanishes at a clearance
  // of epsilon.  field.distances is a DEVICE pointer (DeviceDistanceField), the field trilinear.  trajectory_cost [B];
  // coeff_gradient [B][K][D][N] in the layout of the coefficients (the exact derivative of the sum; yaw rows 0); segment_cost
  // [B][K] (NaN: a segment with more than max_samples samples).  The outputs are optional; without coeff_gradient the kernel
  // without the gradient runs.  false: arguments the call refuses (include/mtg_hip.h).
  bool collisionCost(const mtg_distance_field& field, double dt, double inflation, double epsilon, double speed_epsilon,
                     std::vector<double>* trajectory_cost, std::vector<double>* coeff_gradient = nullptr,
                     std::vector<double>* segment_cost = nullptr, int max_samples = 4096) {
    const size_t n_seg = (size_t)B_ * K_, n_grad = coeff_gradient ? n_seg * D_ * N_ : 0;
    double* d_out = (double*)dmalloc(sizeof(double) * (n_seg + B_ + n_grad));
    const int rc = mtg_collision_cost(ctx(), N_, K_, D_, B_, coeffs_, times_, K_, 1, &field, dt, max_samples, inflation, epsilon,
                                      speed_epsilon, d_out, d_out + n_seg, coeff_gradient ? d_out + n_seg + B_ : nullptr, nullptr);
    if (rc == MTG_OK) {
      if (segment_cost) {
        segment_cost->resize(n_seg);
        check(mtg_copy_to_host(ctx(), segment_cost->data(), d_out, sizeof(double) * n_seg));
      }
      if (trajectory_cost) {
        trajectory_cost->resize(B_);
        check(mtg_copy_to_host(ctx(), trajectory_cost->data(), d_out + n_seg, sizeof(double) * B_));
      }
      if (coeff_gradient) {
        coeff_gradient->resize(n_grad);
        check(mtg_copy_to_host(ctx(), coeff_gradient->data(), d_out + n_seg + B_, sizeof(double) * n_grad));
      }
    }
    mtg_device_free(ctx(), d_out);
    if (rc != MTG_OK && rc != MTG_ERR_INVALID_ARGUMENT) check(rc);
    return rc == MTG_OK;
  }

  // In place on the device copy; returns true when every trajectory ended within range.
  bool scaleSegmentTimesToMeetConstraints(double v_max, double a_max, std::vector<char>* within_range = nullptr,
                                          std::vector<double>* scaling = nullptr) {
    double* ws = (double*)dmalloc(sizeof(double) * 8 * B_ * (K_ + 1));
    double* sc = (double*)dmalloc(sizeof(double) * B_);
    int32_t* within = (int32_t*)dmalloc(sizeof(int32_t) * B_);
    check(mtg_scale_segment_times_to_meet_constraints(ctx(), N_, K_, D_, B_, coeffs_, times_, K_, 1, v_max, a_max,
                                                      /*max_iterations=*/2, ws, sc, within));
    std::vector<int32_t> h(B_);
    check(mtg_copy_to_host(ctx(), h.data(), within, sizeof(int32_t) * h.size()));
    if (scaling) {
      scaling->resize(B_);
      check(mtg_copy_to_host(ctx(), scaling->data(), sc, sizeof(double) * B_));
    }
    mtg_device_free(ctx(), ws);
    mtg_device_free(ctx(), sc);
    mtg_device_free(ctx(), within);
    bool all = true;
    if (within_range) within_range->resize(B_);
    for (int64_t b = 0; b < B_; ++b) {
      all = all && h[b] != 0;
      if (within_range) (*within_range)[b] = (char)(h[b] != 0);
    }
    return all;
  }

  // out[b][i][derivative][dim] at t_start + i*dt, i < n_samples; samples past a trajectory's end are evaluated at
  // its end and excluded from n_valid[b] (the reference's loops simply stop there, src/trajectory.cpp:121-140).
  void sample(double t_start, double dt, int n_samples, int n_derivatives, std::vector<double>* out,
              std::vector<int>* n_valid = nullptr) {
    CHECK_NOTNULL(out);
    const size_t n = (size_t)B_ * n_samples * n_derivatives * D_;
    double* d_out = (double*)dmalloc(sizeof(double) * n);
    int32_t* d_valid = n_valid ? (int32_t*)dmalloc(sizeof(int32_t) * B_) : nullptr;
    check(mtg_sample_range(ctx(), N_, K_, D_, B_, coeffs_, times_, K_, 1, t_start, dt, n_samples, n_derivatives, d_out,
                           d_valid));
    out->resize(n);
    check(mtg_copy_to_host(ctx(), out->data(), d_out, sizeof(double) * n));
    if (n_valid) {
      std::vector<int32_t> h(B_);
      check(mtg_copy_to_host(ctx(), h.data(), d_valid, sizeof(int32_t) * B_));
      n_valid->assign(h.begin(), h.end());
      mtg_device_free(ctx(), d_valid);
    }
    mtg_device_free(ctx(), d_out);
  }

  void download(std::vector<Trajectory>* trajectories) const {
    CHECK_NOTNULL(trajectories);
    std::vector<double> c((size_t)B_ * K_ * D_ * N_), t((size_t)B_ * K_);
    check(mtg_copy_to_host(ctx(), c.data(), coeffs_, sizeof(double) * c.size()));
    check(mtg_copy_to_host(ctx(), t.data(), times_, sizeof(double) * t.size()));
    trajectories->assign(B_, Trajectory());
    for (int64_t b = 0; b < B_; ++b) {
      Segment::Vector segments(K_, Segment(N_, D_));
      for (int k = 0; k < K_; ++k) {
        segments[k].setTime(t[b * K_ + k]);
        for (int d = 0; d < D_; ++d) {
          Eigen::VectorXd v(N_);
          for (int n = 0; n < N_; ++n) v[n] = c[((b * K_ + k) * D_ + d) * N_ + n];
          segments[k][d] = Polynomial(N_, v);
        }
      }
      (*trajectories)[b].setSegments(segments);
    }
  }

 private:
  static mtg_context* ctx() { return mtg_compat_detail::context(); }
  static void check(int rc) { CHECK(rc == MTG_OK) << mtg_status_string(rc) << " " << mtg_last_error_string(ctx()); }
  static void* dmalloc(size_t bytes) {
    void* p = nullptr;
    check(mtg_device_malloc(ctx(), bytes, &p));
    return p;
  }
  void upload(const std::vector<Trajectory>& trajectories) {
    CHECK(!trajectories.empty());
    B_ = (int64_t)trajectories.size();
    N_ = trajectories[0].N();
    K_ = trajectories[0].K();
    D_ = trajectories[0].D();
    std::vector<double> c((size_t)B_ * K_ * D_ * N_), t((size_t)B_ * K_);
    for (int64_t b = 0; b < B_; ++b) {
      const Trajectory& tr = trajectories[b];
      CHECK(tr.N() == N_ && tr.K() == K_ && tr.D() == D_) << "all trajectories of a batch share (N, K, D)";
      for (int k = 0; k < K_; ++k) {
        const Segment& s = tr.segments()[k];
        t[b * K_ + k] = s.getTime();
        for (int d = 0; d < D_; ++d) {
          const Eigen::VectorXd v = s[d].getCoefficients();
          for (int n = 0; n < N_; ++n) c[((b * K_ + k) * D_ + d) * N_ + n] = v[n];
        }
      }
    }
    coeffs_ = (double*)dmalloc(sizeof(double) * c.size());
    times_ = (double*)dmalloc(sizeof(double) * t.size());
    check(mtg_copy_to_device(ctx(), coeffs_, c.data(), sizeof(double) * c.size()));
    check(mtg_copy_to_device(ctx(), times_, t.data(), sizeof(double) * t.size()));
  }
  void release() {
    if (coeffs_) mtg_device_free(ctx(), coeffs_);
    if (times_) mtg_device_free(ctx(), times_);
    coeffs_ = times_ = nullptr;
  }

  int64_t B_ = 0;
  int N_ = 0, K_ = 0, D_ = 0;
  double* coeffs_ = nullptr;   // device [B][K][D][N]
  double* times_ = nullptr;    // device [B][K]
};

// One trajectory against a set of spheres on the HOST (mtg_check_obstacle_clearance_host: no device, no context).  The mtg prefix
// says that this is an addition of this library: the reference has no such function, its callers loop
// Trajectory::offsetTrajectory(-centre) + computeMinMaxMagnitude(POSITION, {0, 1, 2}) over the obstacles.  obstacles = M x (cx, cy,
// cz, r).  Returns the verdict; first_segment / first_obstacle (-1: none) and clearance (the minimum of ||p(t) - c|| - r - inflation
// over the trajectory, NaN wins) are optional.  Arguments the check refuses (no spheres, D not 3 or 4, a negative or non-finite radius
// or inflation): false, with first_segment = first_obstacle = -1 and clearance NaN.
inline bool mtgCheckObstacleClearance(const Trajectory& trajectory, const std::vector<double>& obstacles, double inflation = 0.0,
                                      int* first_segment = nullptr, int* first_obstacle = nullptr, double* clearance = nullptr) {
  const int n = trajectory.N(), k = trajectory.K(), dim = trajectory.D();
  std::vector<double> c((size_t)k * dim * n), t((size_t)k);
  for (int s = 0; s < k; ++s) {
    const Segment& seg = trajectory.segments()[s];
    t[s] = seg.getTime();
    for (int d = 0; d < dim; ++d) {
      const Eigen::VectorXd v = seg[d].getCoefficients();
      for (int i = 0; i < n; ++i) c[((size_t)s * dim + d) * n + i] = v[i];
    }
  }
  int32_t feasible = 0, fseg = -1, fobs = -1;
  double lowest = 0.0;
  const int rc = obstacles.size() % 4 != 0 ? MTG_ERR_INVALID_ARGUMENT
                                            : mtg_check_obstacle_clearance_host(n, k, dim, 1, c.data(), t.data(), k, 1, obstacles.data(),
                                                                                (int32_t)(obstacles.size() / 4), 0, inflation, &feasible, &fseg,
                                                                                &fobs, nullptr, nullptr, nullptr, &lowest);
  if (rc != MTG_OK) {
    feasible = 0;
    fseg = fobs = -1;
    lowest = std::nan("");
  }
  if (first_segment) *first_segment = fseg;
  if (first_obstacle) *first_obstacle = fobs;
  if (clearance) *clearance = lowest;
  return feasible != 0;
}

// Two trajectories against each other on the HOST (mtg_check_trajectory_separation_host: no device, no context); an addition of this
// library like the function above.  start_a / start_b: the global time at which each starts.  Returns the verdict: true iff
// ||a(t) - b(t)|| - min_separation > 0 at every instant both fly (two trajectories that never fly at the same time are apart).
// first_segment_a / _b (the earliest failing piece, -1: none), separation (the minimum, +inf without a common instant, NaN wins) and
// closest_time (its GLOBAL time, NaN: none) are optional.  Arguments the check refuses (different N or D, D not 3 or 4, more than
// 1024 segments, a negative or non-finite min_separation): false, with the indices -1 and separation and closest_time NaN.
inline bool mtgCheckTrajectorySeparation(const Trajectory& a, const Trajectory& b, double min_separation, double start_a = 0.0,
                                         double start_b = 0.0, int* first_segment_a = nullptr, int* first_segment_b = nullptr,
                                         double* separation = nullptr, double* closest_time = nullptr) {
  const int n = a.N(), dim = a.D();
  auto flat = [&](const Trajectory& trajectory, std::vector<double>& c, std::vector<double>& t) {
    const int k = trajectory.K();
    c.resize((size_t)k * dim * n);
    t.resize((size_t)k);
    for (int s = 0; s < k; ++s) {
      const Segment& seg = trajectory.segments()[s];
      t[s] = seg.getTime();
      for (int d = 0; d < dim; ++d) {
        const Eigen::VectorXd v = seg[d].getCoefficients();
        for (int i = 0; i < n; ++i) c[((size_t)s * dim + d) * n + i] = v[i];
      }
    }
  };
  int32_t feasible = 0, fa = -1, fb = -1, ca = -1, cb = -1;
  double lowest = 0.0, when = 0.0;
  int rc = MTG_ERR_INVALID_ARGUMENT;
  if (b.N() == n && b.D() == dim && a.K() >= 1 && b.K() >= 1) {
    std::vector<double> c_a, t_a, c_b, t_b;
    flat(a, c_a, t_a);
    flat(b, c_b, t_b);
    const int32_t pair[2] = {0, 0};
    std::vector<double> seg_sep((size_t)a.K()), seg_time((size_t)a.K());
    std::vector<int32_t> seg_b((size_t)a.K());
    rc = mtg_check_trajectory_separation_host(n, dim, a.K(), 1, c_a.data(), t_a.data(), a.K(), 1, &start_a, b.K(), 1, c_b.data(), t_b.data(),
                                              b.K(), 1, &start_b, 1, pair, min_separation, &feasible, &fa, &fb, &lowest, &when, &ca, &cb,
                                              seg_sep.data(), seg_time.data(), seg_b.data(), nullptr);
  }
  if (rc != MTG_OK) {
    feasible = 0;
    fa = fb = -1;
    lowest = when = std::nan("");
  }
  if (first_segment_a) *first_segment_a = fa;
  if (first_segment_b) *first_segment_b = fb;
  if (separation) *separation = lowest;
  if (closest_time) *closest_time = when;
  return feasible != 0;
}

// One trajectory against a set of convex keep-out zones on the HOST (mtg_check_keep_out_zones_host: no device, no context); an
// addition of this library like the function above.  zones = M x n_planes x (nx, ny, nz, offset) as in
// TrajectoryBatch::checkKeepOutZones.  Returns the verdict; first_segment / first_zone (-1: none) and clearance (the minimum over the
// trajectory, NaN wins) are optional.  Arguments the check refuses (no zones, n_planes not in 1 .. 8, D not 3 or 4, a normal that is
// not of unit length, an offset or inflation that is not finite, a negative inflation): false, with first_segment = first_zone = -1
// and clearance NaN.
inline bool mtgCheckKeepOutZones(const Trajectory& trajectory, const std::vector<double>& zones, int n_planes, double inflation = 0.0,
                                 int* first_segment = nullptr, int* first_zone = nullptr, double* clearance = nullptr) {
  const int n = trajectory.N(), k = trajectory.K(), dim = trajectory.D();
  std::vector<double> c((size_t)k * dim * n), t((size_t)k);
  for (int s = 0; s < k; ++s) {
    const Segment& seg = trajectory.segments()[s];
    t[s] = seg.getTime();
    for (int d = 0; d < dim; ++d) {
      const Eigen::VectorXd v = seg[d].getCoefficients();
      for (int i = 0; i < n; ++i) c[((size_t)s * dim + d) * n + i] = v[i];
    }
  }
  int32_t feasible = 0, fseg = -1, fzone = -1;
  double lowest = 0.0;
  const bool whole = n_planes >= 1 && n_planes <= 8 && zones.size() % (4 * (size_t)n_planes) == 0;
  const int rc = !whole ? MTG_ERR_INVALID_ARGUMENT
                        : mtg_check_keep_out_zones_host(n, k, dim, 1, c.data(), t.data(), k, 1, zones.data(),
                                                        (int32_t)(zones.size() / (4 * (size_t)n_planes)), n_planes, 0, inflation, &feasible,
                                                        &fseg, &fzone, nullptr, nullptr, nullptr, &lowest);
  if (rc != MTG_OK) {
    feasible = 0;
    fseg = fzone = -1;
    lowest = std::nan("");
  }
  if (first_segment) *first_segment = fseg;
  if (first_zone) *first_zone = fzone;
  if (clearance) *clearance = lowest;
  return feasible != 0;
}

// A voxel grid of distances on the device for TrajectoryBatch::checkDistanceField: the grid of a HOST mtg_distance_field is
// uploaded once, field() is the same description with the device pointer.  Owns the device copy.
class DeviceDistanceField {
 public:
  explicit DeviceDistanceField(const mtg_distance_field& host) : field_(host) {
    const size_t bytes = sizeof(float) * (size_t)host.nx * (size_t)host.ny * (size_t)host.nz;
    void* p = nullptr;
    CHECK(host.distances != nullptr && host.nx > 0 && host.ny > 0 && host.nz > 0);
    CHECK(mtg_device_malloc(mtg_compat_detail::context(), bytes, &p) == MTG_OK);
    CHECK(mtg_copy_to_device(mtg_compat_detail::context(), p, host.distances, bytes) == MTG_OK);
    field_.distances = (const float*)p;
  }
  DeviceDistanceField(const DeviceDistanceField&) = delete;
  DeviceDistanceField& operator=(const DeviceDistanceField&) = delete;
  ~DeviceDistanceField() { mtg_device_free(mtg_compat_detail::context(), (void*)field_.distances); }
  const mtg_distance_field& field() const { return field_; }

 private:
  mtg_distance_field field_;
};

// One trajectory against a voxel grid of distances on the HOST (mtg_check_distance_field_host: no device, no context); an addition
// of this library like the functions above.  field.distances is a host pointer.  A SAMPLED check: every segment at local times 0,
// i dt < T and T.  Returns the verdict; first_segment (-1: none), first_time (the local time of the first failing sample of that
// segment; NaN: none, or that segment has more than max_samples samples) and clearance (the minimum of distance - inflation over the
// samples, NaN wins) are optional.  Arguments the check refuses (include/mtg_hip.h): false, with first_segment = -1, first_time and
// clearance NaN.
inline bool mtgCheckDistanceField(const Trajectory& trajectory, const mtg_distance_field& field, double dt, double inflation = 0.0,
                                  int* first_segment = nullptr, double* first_time = nullptr, double* clearance = nullptr,
                                  int max_samples = 4096) {
  const int n = trajectory.N(), k = trajectory.K(), dim = trajectory.D();
  std::vector<double> c((size_t)k * dim * n), t((size_t)k);
  for (int s = 0; s < k; ++s) {
    const Segment& seg = trajectory.segments()[s];
    t[s] = seg.getTime();
    for (int d = 0; d < dim; ++d) {
      const Eigen::VectorXd v = seg[d].getCoefficients();
      for (int i = 0; i < n; ++i) c[((size_t)s * dim + d) * n + i] = v[i];
    }
  }
  int32_t feasible = 0, fseg = -1;
  double lowest = 0.0, ftime = std::nan("");
  std::vector<int32_t> failing((size_t)k), samples((size_t)k);
  const int rc = mtg_check_distance_field_host(n, k, dim, 1, c.data(), t.data(), k, 1, &field, dt, max_samples, inflation, &feasible, &fseg,
                                               nullptr, nullptr, failing.data(), samples.data(), &lowest);
  if (rc != MTG_OK) {
    feasible = 0;
    fseg = -1;
    lowest = std::nan("");
  } else if (fseg >= 0 && failing[fseg] >= 0) {
    ftime = failing[fseg] == samples[fseg] - 1 ? t[fseg] : (double)failing[fseg] * dt;
  }
  if (first_segment) *first_segment = fseg;
  if (first_time) *first_time = ftime;
  if (clearance) *clearance = lowest;
  return feasible != 0;
}

// One trajectory against a trilinear voxel grid of distances on the HOST, CERTIFIED (mtg_certify_distance_field_host: no device, no
// context): a verdict for every instant.  lipschitz <= 0: computed from the grid (mtg_distance_field_lipschitz_host).  Returns the
// result code (MTG_FIELD_COLLIDES 0, MTG_FIELD_FREE 1, MTG_FIELD_UNDECIDED_DEPTH 2, MTG_FIELD_UNDECIDED_BUDGET 3) of the first
// segment that is not FREE; first_segment (-1: none), first_time (the local time of the first failing sample of that segment; NaN:
// none), lower_bound (guaranteed, of the minimum of distance - inflation) and sampled_clearance (the lowest sample) are optional.
// Arguments the check refuses (include/mtg_hip.h): -1, with first_segment = -1 and the three values NaN.
inline int mtgCertifyDistanceField(const Trajectory& trajectory, const mtg_distance_field& field, double lipschitz = 0.0,
                                   double inflation = 0.0, int* first_segment = nullptr, double* first_time = nullptr,
                                   double* lower_bound = nullptr, double* sampled_clearance = nullptr, int min_depth = 4, int max_depth = 16,
                                   int max_frontier = 1024) {
  const int n = trajectory.N(), k = trajectory.K(), dim = trajectory.D();
  std::vector<double> c((size_t)k * dim * n), t((size_t)k);
  for (int s = 0; s < k; ++s) {
    const Segment& seg = trajectory.segments()[s];
    t[s] = seg.getTime();
    for (int d = 0; d < dim; ++d) {
      const Eigen::VectorXd v = seg[d].getCoefficients();
      for (int i = 0; i < n; ++i) c[((size_t)s * dim + d) * n + i] = v[i];
    }
  }
  int32_t result = -1, fseg = -1;
  double lower = std::nan(""), sampled = std::nan(""), ftime = std::nan("");
  std::vector<double> failing((size_t)k);
  int rc = MTG_OK;
  if (!(lipschitz > 0.0)) rc = mtg_distance_field_lipschitz_host(&field, &lipschitz);
  if (rc == MTG_OK)
    rc = mtg_certify_distance_field_host(n, k, dim, 1, c.data(), t.data(), k, 1, &field, lipschitz, min_depth, max_depth, max_frontier,
                                         inflation, &result, &fseg, nullptr, nullptr, nullptr, nullptr, failing.data(), nullptr, nullptr,
                                         &lower, &sampled);
  if (rc != MTG_OK) {
    result = -1;
    fseg = -1;
    lower = sampled = std::nan("");
  } else if (fseg >= 0) {
    ftime = failing[fseg];
  }
  if (first_segment) *first_segment = fseg;
  if (first_time) *first_time = ftime;
  if (lower_bound) *lower_bound = lower;
  if (sampled_clearance) *sampled_clearance = sampled;
  return result;
}

// TrajectoryBatch::collisionCost on a DeviceDistanceField (the device copy of a host grid).
inline bool mtgCollisionCost(TrajectoryBatch& batch, const DeviceDistanceField& field, double dt, double inflation, double epsilon,
                             double speed_epsilon, std::vector<double>* trajectory_cost, std::vector<double>* coeff_gradient = nullptr,
                             std::vector<double>* segment_cost = nullptr, int max_samples = 4096) {
  return batch.collisionCost(field.field(), dt, inflation, epsilon, speed_epsilon, trajectory_cost, coeff_gradient, segment_cost, max_samples);
}

// One trajectory's distance-field collision cost and gradient on the HOST (mtg_collision_cost_host: no device, no context; the
// same order of every sum as the device form).  field.distances is a host pointer, the field trilinear.  Returns the trajectory's
// cost; coeff_gradient [K][D][N] (the layout of the segments' coefficients) and segment_cost [K] are optional.  Arguments the call
// refuses (include/mtg_hip.h): NaN, and the two vectors are emptied.
inline double mtgCollisionCost(const Trajectory& trajectory, const mtg_distance_field& field, double dt, double inflation, double epsilon,
                               double speed_epsilon = 1e-3, std::vector<double>* coeff_gradient = nullptr,
                               std::vector<double>* segment_cost = nullptr, int max_samples = 4096) {
  const int n = trajectory.N(), k = trajectory.K(), dim = trajectory.D();
  std::vector<double> c((size_t)k * dim * n), t((size_t)k), seg((size_t)k);
  for (int s = 0; s < k; ++s) {
    const Segment& segment = trajectory.segments()[s];
    t[s] = segment.getTime();
    for (int d = 0; d < dim; ++d) {
      const Eigen::VectorXd v = segment[d].getCoefficients();
      for (int i = 0; i < n; ++i) c[((size_t)s * dim + d) * n + i] = v[i];
    }
  }
  double total = std::nan("");
  if (coeff_gradient) coeff_gradient->assign(c.size(), 0.0);
  const int rc = mtg_collision_cost_host(n, k, dim, 1, c.data(), t.data(), k, 1, &field, dt, max_samples, inflation, epsilon, speed_epsilon,
                                         seg.data(), &total, coeff_gradient ? coeff_gradient->data() : nullptr, nullptr);
  if (rc != MTG_OK) {
    total = std::nan("");
    seg.clear();
    if (coeff_gradient) coeff_gradient->clear();
  }
  if (segment_cost) *segment_cost = seg;
  return total;
}

}  // namespace mav_trajectory_generation
#endif
