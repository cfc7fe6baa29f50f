// shot_math.hpp -- the arithmetic of the SHOT352 descriptor pipeline (reference src/comparator.cpp:941-986: processSHOT's
// deterministic part = pcl::NormalEstimation, removeNaNNormalsFromPointCloud, pcl::SHOTEstimation<PointXYZRGB, Normal, SHOT352>),
// shared by the device kernels (shot.hip) and the host mirror of the tests (tests/cpp/shot_host.cpp).  Unfused
// (-ffp-contract=off), correctly rounded '/', sqrtf and sqrt on both sides, lm_acos and lm_atan2 (libm_f64.hpp) for the two
// transcendentals, float where PCL's expressions are float and double where they promote: the device returns the host's bits.
// The PCL details are [recalled] from the published source of PCL 1.7 (shot.hpp, shot_lrf.hpp): PCL is not
// available to compare against, parity with it is unpinned.
#pragma once
#include "libm_f32.hpp"
#include "libm_f64.hpp"

namespace pcc {

constexpr int SHOT_SHAPE_BINS = 10;                          // nr_shape_bins_
constexpr int SHOT_VOLUME_BINS = SHOT_SHAPE_BINS + 1;        // the slots of one volume
constexpr int SHOT_VOLUMES = 32;                             // nr_grid_sector_ = maxAngularSectors_: 8 azimuth x 2 elevation x 2 radial
constexpr int SHOT_BINS = SHOT_VOLUMES * SHOT_VOLUME_BINS;   // pcl::SHOT352::descriptor
constexpr int SHOT_MIN_NEIGHBOURS = 5;                       // both "fewer than 5" rules
constexpr int SHOT_JACOBI_SWEEPS = 32;                       // the sweep cap of shot_jacobi3
// PCL's PST_* literals
constexpr double SHOT_RAD_45 = 0.78539816339744830961566084581988;
constexpr double SHOT_RAD_90 = 1.5707963267948966192313216916398;
constexpr double SHOT_RAD_135 = 2.3561944901923449288469825374596;
constexpr double SHOT_RAD_PI_7_8 = 2.7488935718910690836548129603691;

__host__ __device__ inline bool shot_finite(float f) { return (lm_bits(f) & 0x7f800000u) != 0x7f800000u; }
__host__ __device__ inline bool shot_finite(double d) { return (lm_bits64(d) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }
__host__ __device__ inline float shot_nan() { return lm_float(0x7fc00000u); }

// a float dot in storage order: ((x x' + y y') + z z')
__host__ __device__ inline float shot_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
// the same in double (the sign votes of the LRF)
__host__ __device__ inline double shot_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// ---- the local reference frame (SHOTLocalReferenceFrameEstimation::getLocalRF) ------------------------------------------------
// One row entry q of p with d2 != 0: v = double(q - p) (the difference in float), and the seven terms it adds, in the order
// xx, xy, xz, yy, yz, zz, w: w * (v_i * v_j) and w = double(r) - double(sqrtf(d2)).
__host__ __device__ inline void shot_lrf_term(const float p[3], const float q[3], float d2, double r, double v[3], double t[7]) {
    for (int k = 0; k < 3; ++k) v[k] = (double)(q[k] - p[k]);
    const double w = r - (double)sqrtf(d2);
    t[0] = w * (v[0] * v[0]);
    t[1] = w * (v[0] * v[1]);
    t[2] = w * (v[0] * v[2]);
    t[3] = w * (v[1] * v[1]);
    t[4] = w * (v[1] * v[2]);
    t[5] = w * (v[2] * v[2]);
    t[6] = w;
}
// acc += the terms of one entry; the entries come in row order, and that order is part of the result
__host__ __device__ inline void shot_lrf_accumulate(double acc[7], const float p[3], const float q[3], float d2, double r, double v[3]) {
    double t[7];
    shot_lrf_term(p, q, d2, r, v, t);
    for (int k = 0; k < 7; ++k) acc[k] += t[k];
}

// one rotation of shot_jacobi3 (below) on the pair (p, q), o the third index; the indices are constants at every call
__host__ __device__ inline void shot_jacobi_rotate(double m[3][3], double V[3][3], const int p, const int q, const int o) {
    const double apq = m[p][q];
    if (apq == 0.0) return;
    const double mag = lm_abs(apq), dp = lm_abs(m[p][p]), dq = lm_abs(m[q][q]);
    if (dp + mag == dp && dq + mag == dq) { m[p][q] = m[q][p] = 0.0; return; }  // below half an ulp of both diagonal entries
    const double theta = (m[q][q] - m[p][p]) / (2.0 * apq);
    const double den = lm_abs(theta) + sqrt(theta * theta + 1.0);
    const double t = theta < 0.0 ? -1.0 / den : 1.0 / den;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    m[p][p] = m[p][p] - t * apq;
    m[q][q] = m[q][q] + t * apq;
    m[p][q] = m[q][p] = 0.0;
    const double aop = m[o][p], aoq = m[o][q];
    m[o][p] = m[p][o] = c * aop - s * aoq;
    m[o][q] = m[q][o] = s * aop + c * aoq;
    for (int k = 0; k < 3; ++k) {
        const double vkp = V[k][p], vkq = V[k][q];
        V[k][p] = c * vkp - s * vkq;
        V[k][q] = s * vkp + c * vkq;
    }
}
// Eigenvalues d[3] and eigenvectors (column k of V = V[0][k], V[1][k], V[2][k]) of the symmetric 3 x 3 matrix
// a = {xx, xy, xz, yy, yz, zz}: cyclic Jacobi in double from + - * / sqrt alone.  A sweep rotates (0,1), (0,2), (1,2) in this
// order, skipping an off-diagonal that is exactly 0.0; an off-diagonal that changes neither of its diagonal entries when its
// magnitude is added to theirs (|a_pp| + |a_pq| == |a_pp| and |a_qq| + |a_pq| == |a_qq|) is set to 0.0 without a rotation
// (between equal eigenvalues a rotation by 45 degrees would carry it round for ever); a rotation takes theta = (a_qq - a_pp) / (2 a_pq),
// t = sign(theta) / (|theta| + sqrt(theta^2 + 1)) (sign(0) = +1), c = 1 / sqrt(t^2 + 1), s = t c, sets a_pq to 0.0 and updates
// a_pp -= t a_pq, a_qq += t a_pq, the third row / column and V.  It stops when all three off-diagonals are exactly 0.0 (the
// convergence is quadratic and ends in underflow) or after SHOT_JACOBI_SWEEPS sweeps; returns the sweeps it took, or
// SHOT_JACOBI_SWEEPS + 1 when the cap was hit (the diagonal and V are then used as they stand).
__host__ __device__ inline int shot_jacobi3(const double a[6], double d[3], double V[3][3]) {
    double m[3][3] = {{a[0], a[1], a[2]}, {a[1], a[3], a[4]}, {a[2], a[4], a[5]}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    int sweep = 0;
    for (; sweep <= SHOT_JACOBI_SWEEPS; ++sweep) {
        if (m[0][1] == 0.0 && m[0][2] == 0.0 && m[1][2] == 0.0) break;
        if (sweep == SHOT_JACOBI_SWEEPS) { ++sweep; break; }
        shot_jacobi_rotate(m, V, 0, 1, 2);  // (constant indices: the matrices stay in registers on the device)
        shot_jacobi_rotate(m, V, 0, 2, 1);
        shot_jacobi_rotate(m, V, 1, 2, 0);
    }
    d[0] = m[0][0]; d[1] = m[1][1]; d[2] = m[2][2];
    return sweep;
}

// The unsigned x and z axes from the sums of a row (acc as shot_lrf_accumulate leaves them): cov = acc[k] / sum, a true division
// per entry; shot_jacobi3; then PCL's if-chain over the three eigenvalues e0, e1, e2 as the solver holds them, every comparison a
// strict '>': e0 > e1 ? (e0 > e2 ? x = col 0, z = (e1 > e2 ? col 2 : col 1) : x = col 2, z = col 1)
//                     : (e1 > e2 ? x = col 1, z = (e0 > e2 ? col 2 : col 0) : x = col 2, z = col 0)
// -- among equal eigenvalues the LATER column is the larger for x, and z takes what the chain leaves.  false: an eigenvalue is not
// finite (a zero or non-finite sum), the frame is NaN.
__host__ __device__ inline bool shot_lrf_axes(const double acc[7], double x[3], double z[3]) {
    double cov[6], e[3], V[3][3];
    for (int k = 0; k < 6; ++k) cov[k] = acc[k] / acc[6];
    shot_jacobi3(cov, e, V);
    if (!shot_finite(e[0]) || !shot_finite(e[1]) || !shot_finite(e[2])) return false;
    int cx, cz;
    if (e[0] > e[1]) {
        if (e[0] > e[2]) { cx = 0; cz = e[1] > e[2] ? 2 : 1; }
        else { cx = 2; cz = 1; }
    } else {
        if (e[1] > e[2]) { cx = 1; cz = e[0] > e[2] ? 2 : 0; }
        else { cx = 2; cz = 0; }
    }
    for (int k = 0; k < 3; ++k) {
        x[k] = cx == 0 ? V[k][0] : cx == 1 ? V[k][1] : V[k][2];
        z[k] = cz == 0 ? V[k][0] : cz == 1 ? V[k][1] : V[k][2];
    }
    return true;
}

// The sign rule of one axis from its votes over the `valid` entries kept in row order: plus = the entries with v . axis >= 0,
// median_plus = those with v . axis > 0 among the five entries valid / 2 - 2 .. valid / 2 + 2 of that list.  true: negate.
__host__ __device__ inline bool shot_sign_negate(int plus, int valid, int median_plus) {
    const int s = 2 * plus - valid;
    if (s < 0) return true;
    if (s == 0) return median_plus < 3;
    return false;
}
// whether list position `at` belongs to the five median entries
__host__ __device__ inline bool shot_sign_median(int at, int valid) { return at >= valid / 2 - 2 && at <= valid / 2 + 2; }

// both axes signed in place: v = the `valid` (>= 5) difference vectors of the row, 3 doubles each, in row order
__host__ __device__ inline void shot_lrf_signs(const double* v, int valid, double x[3], double z[3]) {
    int plus_x = 0, plus_z = 0, med_x = 0, med_z = 0;
    for (int e = 0; e < valid; ++e) {
        const double dx = shot_dot(v + 3 * e, x), dz = shot_dot(v + 3 * e, z);
        if (dx >= 0.0) ++plus_x;
        if (dz >= 0.0) ++plus_z;
        if (shot_sign_median(e, valid)) {
            if (dx > 0.0) ++med_x;
            if (dz > 0.0) ++med_z;
        }
    }
    if (shot_sign_negate(plus_x, valid, med_x)) for (int k = 0; k < 3; ++k) x[k] = x[k] * -1.0;
    if (shot_sign_negate(plus_z, valid, med_z)) for (int k = 0; k < 3; ++k) z[k] = z[k] * -1.0;
}

// rf rows: float(x), y = z cross x in float, float(z)
__host__ __device__ inline void shot_rf(const double x[3], const double z[3], float rf[9]) {
    for (int k = 0; k < 3; ++k) { rf[k] = (float)x[k]; rf[6 + k] = (float)z[k]; }
    const float *a = rf + 6, *b = rf;
    rf[3] = a[1] * b[2] - a[2] * b[1];
    rf[4] = a[2] * b[0] - a[0] * b[2];
    rf[5] = a[0] * b[1] - a[1] * b[0];
}
__host__ __device__ inline void shot_rf_nan(float rf[9]) { for (int k = 0; k < 9; ++k) rf[k] = shot_nan(); }

// ---- one row entry of the descriptor (computePointSHOT + interpolateSingleChannel) ----------------------------------------------
// p and its frame rf, the entry q with its normal nq at squared distance d2, r the double shot_radius.  Returns false when the entry
// is skipped (|distance| < 1e-15); else bin[0 .. 4] / val[0 .. 4]: the contributions in the order they are added -- the cosine
// neighbour, the radial neighbour, the inclination neighbour, the azimuth neighbour, the centre bin -- bin[k] = -1 for one that
// PCL does not apply.
__host__ __device__ inline bool shot_entry(const float p[3], const float rf[9], const float q[3], const float nq[3], float d2, double r,
                                           int bin[5], float val[5]) {
    const double distance = (double)sqrtf(d2);
    if (lm_abs(distance) < 1e-15) return false;
    const double r1_2 = r / 2, r3_4 = (r * 3) / 4, r1_4 = r / 4;
    double cosine = (double)shot_dot(nq, rf + 6);
    if (cosine > 1.0) cosine = 1.0;
    if (cosine < -1.0) cosine = -1.0;
    double bd = ((1.0 + cosine) * SHOT_SHAPE_BINS) / 2;
    const float delta[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
    double xF = (double)shot_dot(delta, rf), yF = (double)shot_dot(delta, rf + 3), zF = (double)shot_dot(delta, rf + 6);
    if (lm_abs(yF) < 1E-30) yF = 0;
    if (lm_abs(xF) < 1E-30) xF = 0;
    if (lm_abs(zF) < 1E-30) zF = 0;
    const int bit4 = ((yF > 0) || ((yF == 0.0) && (xF < 0))) ? 1 : 0;
    const int bit3 = ((xF > 0) || ((xF == 0.0) && (yF > 0))) ? !bit4 : bit4;
    int desc = ((bit4 << 3) + (bit3 << 2)) << 1;
    if ((xF * yF > 0) || (xF == 0.0)) desc += (lm_abs(xF) >= lm_abs(yF)) ? 0 : 4;
    else desc += (lm_abs(xF) > lm_abs(yF)) ? 4 : 0;
    desc += zF > 0 ? 1 : 0;
    desc += (distance > r1_2) ? 2 : 0;
    const int step = (int)floor(bd + 0.5);
    const int volume = desc * SHOT_VOLUME_BINS;
    for (int k = 0; k < 4; ++k) { bin[k] = -1; val[k] = 0.f; }
    // the cosine (adjacent bins of the volume)
    bd -= step;
    double weight = 1 - lm_abs(bd);
    bin[0] = volume + (bd > 0 ? (step + 1) % SHOT_SHAPE_BINS : (step - 1 + SHOT_SHAPE_BINS) % SHOT_SHAPE_BINS);
    val[0] = (float)lm_abs(bd);
    // the distance (adjacent husks)
    if (distance > r1_2) {
        const double rd = (distance - r3_4) / r1_2;
        if (distance > r3_4) weight += 1 - rd;
        else { weight += 1 + rd; bin[1] = (desc - 2) * SHOT_VOLUME_BINS + step; val[1] = (float)lm_abs(rd); }
    } else {
        const double rd = (distance - r1_4) / r1_2;
        if (distance < r1_4) weight += 1 + rd;
        else { weight += 1 - rd; bin[1] = (desc + 2) * SHOT_VOLUME_BINS + step; val[1] = (float)lm_abs(rd); }
    }
    // the inclination (adjacent vertical volumes)
    double ic = zF / distance;
    if (ic < -1.0) ic = -1.0;
    if (ic > 1.0) ic = 1.0;
    const double inclination = lm_acos(ic);
    if (inclination > SHOT_RAD_90 || (lm_abs(inclination - SHOT_RAD_90) < 1e-30 && zF <= 0)) {
        const double id = (inclination - SHOT_RAD_135) / SHOT_RAD_90;
        if (inclination > SHOT_RAD_135) weight += 1 - id;
        else { weight += 1 + id; bin[2] = (desc + 1) * SHOT_VOLUME_BINS + step; val[2] = (float)lm_abs(id); }
    } else {
        const double id = (inclination - SHOT_RAD_45) / SHOT_RAD_90;
        if (inclination < SHOT_RAD_45) weight += 1 + id;
        else { weight += 1 - id; bin[2] = (desc - 1) * SHOT_VOLUME_BINS + step; val[2] = (float)lm_abs(id); }
    }
    // the azimuth (adjacent horizontal volumes)
    if (yF != 0.0 || xF != 0.0) {
        const double azimuth = lm_atan2(yF, xF);
        const int sel = desc >> 2;
        double ad = (azimuth - (-SHOT_RAD_PI_7_8 + SHOT_RAD_45 * sel)) / SHOT_RAD_45;
        if (ad > 0.5) ad = 0.5;
        if (ad < -0.5) ad = -0.5;
        if (ad > 0) {
            weight += 1 - ad;
            bin[3] = ((desc + 4) % SHOT_VOLUMES) * SHOT_VOLUME_BINS + step;
        } else {
            weight += 1 + ad;
            bin[3] = ((desc - 4 + SHOT_VOLUMES) % SHOT_VOLUMES) * SHOT_VOLUME_BINS + step;
        }
        val[3] = (float)lm_abs(ad);
    }
    bin[4] = volume + step;
    val[4] = (float)weight;
    return true;
}

// float(sqrt(sum of double(b) * double(b))) over the 352 bins in index order, one chain in double: every bin is then divided by it
__host__ __device__ inline float shot_norm(const float* bins) {
    double acc = 0.0;
    for (int b = 0; b < SHOT_BINS; ++b) acc += (double)bins[b] * (double)bins[b];
    return (float)sqrt(acc);
}

}  // namespace pcc
