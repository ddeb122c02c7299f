// Torsion matching of ligand conformers (the second half of the reference's conformer matching:
// datasets/conformer_matching.py:30-61 as used at datasets/process_mols.py:624-650).  For a probe conformer and a target (holo) pose of
// the same molecule, find the R dihedral angles theta that minimise
//     f(theta) = min over rigid motions of RMSD(probe with its R dihedrals SET to theta, target).
// Every torsion bond is a bridge, so the dihedrals are independent: the probe's own dihedral phi_r is computed once and the rotating side
// of bond r (mask_rotate row r) is turned by +-(theta_r - phi_r) about the bond axis, r = 0 .. R-1 in order, with the rotation arithmetic
// of pose_update_kernel (kernels.hip; axis_angle_to_matrix of pose_math.h).  The aligned RMSD is closed form:
// rmsd^2 = (sum|a|^2 + sum|b|^2 - 2 lambda_max) / Nl on centred coordinates, lambda_max = the largest eigenvalue of Horn's 4x4 matrix
// (horn_lambda_max of pose_math.h: fp64 Jacobi without eigenvectors).  Dihedral convention: IUPAC / rdkit -- cis 0, trans pi, looking down u -> v a clockwise turn of l relative to k is positive.
//
// match_score_kernel: f for given theta vectors, one wave per (problem, theta), one lane per atom (strided for Nl > 64).
// match_de_kernel:    the whole differential evolution of one problem in one workgroup of 4 waves, population / trials / fitness in LDS,
//                     generation-synchronous (what scipy calls updating='deferred'), no host round trip.
// A wave keeps its atoms (probe, centred target, per-atom bit mask of the bonds that move it) in registers; the two axis atoms of a
// rotation are fetched from their owning lanes with a shuffle, so the objective needs no LDS and no barrier.
// Latency-bound, no matrix-core work; the gain is P individuals x many problems at once.  No atomics, no random state in memory:
// every draw is a hash of (seed, problem id, generation, individual, dimension, purpose), so the result does not depend on which wave
// evaluates which individual nor on what else shares the launch.
#include <hip/hip_runtime.h>

#include <atomic>

#include "device_util.h"
#include "host_util.h"
#include "pose_math.h"

namespace cbd {

constexpr int TM_MAX_R = 32;       // one bit per bond in the per-atom mask, one lane per bond for phi / theta
constexpr int TM_MAX_NL = 256;     // 4 atoms per lane
constexpr int TM_SLOTS = TM_MAX_NL / 64;
constexpr int TM_MAX_POP = 512;    // popsize * R
constexpr int TM_WAVES = 4;
constexpr int TM_MIN_POP = 5;      // best1bin needs the candidate, the best and two more
constexpr float TM_PI = 3.14159265358979323846f;

struct MatchProblems {
  int n, max_nl, max_r;
  const int* nl;                  // [n] or null (= max_nl)
  const int* r;                   // [n] or null (= max_r)
  const float* probe;             // [n][max_nl][3]
  const float* target;            // [n][max_nl][3]
  const int* quads;               // [n][max_r][4]  (k, u, v, l)
  const unsigned char* mask;      // [n][max_r][max_nl]
};

struct DeParams {
  const int* problem_id;          // [n] or null (= index in the launch): part of the random-number key
  unsigned long long seed;
  int popsize, maxiter;
  float mut_lo, mut_hi, recombination, tol;
  float* theta_out;               // [n][max_r]
  float* fitness_out;             // [n]
  int* gens_out;                  // [n]
};

// IUPAC dihedral of four points
CBD_DEV float dihedral4(const float* p0, const float* p1, const float* p2, const float* p3) {
  const float b1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  const float b2[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  const float b3[3] = {p3[0] - p2[0], p3[1] - p2[1], p3[2] - p2[2]};
  const float n1[3] = {b1[1] * b2[2] - b1[2] * b2[1], b1[2] * b2[0] - b1[0] * b2[2], b1[0] * b2[1] - b1[1] * b2[0]};
  const float n2[3] = {b2[1] * b3[2] - b2[2] * b3[1], b2[2] * b3[0] - b2[0] * b3[2], b2[0] * b3[1] - b2[1] * b3[0]};
  const float m[3] = {n1[1] * n2[2] - n1[2] * n2[1], n1[2] * n2[0] - n1[0] * n2[2], n1[0] * n2[1] - n1[1] * n2[0]};
  const float nb2 = sqrtf(b2[0] * b2[0] + b2[1] * b2[1] + b2[2] * b2[2]);
  const float y = (m[0] * b2[0] + m[1] * b2[1] + m[2] * b2[2]) / nb2;
  const float x = n1[0] * n2[0] + n1[1] * n2[1] + n1[2] * n2[2];
  return atan2f(y, x);
}

// a[s] for a wave-uniform s.  Written with bit masks: a chain of selects is folded back into a dynamically indexed array by the
// compiler, which then keeps the coordinates in memory instead of registers
CBD_DEV float slot_pick(const float (&a)[TM_SLOTS], int s) {
  unsigned t = 0u;
#pragma unroll
  for (int k = 0; k < TM_SLOTS; ++k) t |= __float_as_uint(a[k]) & (s == k ? 0xffffffffu : 0u);
  return __uint_as_float(t);
}

// One matching problem as a wave holds it.  Lane L owns atoms L, L + 64, ... ; lane r < R also owns bond r (phi, axis atoms, sign).
struct WaveProblem {
  float px[TM_SLOTS], py[TM_SLOTS], pz[TM_SLOTS];   // probe
  float tx[TM_SLOTS], ty[TM_SLOTS], tz[TM_SLOTS];   // centred target
  unsigned rot[TM_SLOTS];                           // bit r: bond r moves this atom
  float phi, sgn;                                   // of bond `lane`
  int uv;                                           // u | v << 16 of bond `lane`
  double tb2;                                       // sum |b|^2 of the centred target
  int nl, R, nslots;
  bool ok;

  // false (for the whole wave) when the description is outside the limits or an index is out of range; nothing is read out of bounds
  CBD_DEV bool load(const MatchProblems& mp, int p) {
    const int lane = lane_id();
    nl = mp.nl ? mp.nl[p] : mp.max_nl;
    R = mp.r ? mp.r[p] : mp.max_r;
    nslots = 0;
    phi = 0.f; sgn = 0.f; uv = 0; tb2 = 0.0;
#pragma unroll
    for (int s = 0; s < TM_SLOTS; ++s) { px[s] = py[s] = pz[s] = tx[s] = ty[s] = tz[s] = 0.f; rot[s] = 0u; }
    ok = nl >= 1 && nl <= mp.max_nl && mp.max_nl <= TM_MAX_NL && R >= 1 && R <= mp.max_r && mp.max_r <= TM_MAX_R;
    if (!ok) return false;
    nslots = (nl + 63) >> 6;
    const float* P = mp.probe + (size_t)p * mp.max_nl * 3;
    const float* T = mp.target + (size_t)p * mp.max_nl * 3;
    const int* Q = mp.quads + (size_t)p * mp.max_r * 4;
    const unsigned char* M = mp.mask + (size_t)p * mp.max_r * mp.max_nl;
    bool good = true;
    if (lane < R) {
      const int k = Q[4 * lane], u = Q[4 * lane + 1], v = Q[4 * lane + 2], l = Q[4 * lane + 3];
      good = k >= 0 && k < nl && u >= 0 && u < nl && v >= 0 && v < nl && l >= 0 && l < nl && u != v;
      if (good) {
        const bool mk = M[(size_t)lane * mp.max_nl + k] != 0, ml = M[(size_t)lane * mp.max_nl + l] != 0;
        good = mk != ml;   // exactly one side of the bond rotates
        // the rotation is about the direction u - v (pose_update_kernel): it lowers the dihedral when the l side turns
        sgn = ml ? -1.f : 1.f;
        uv = u | (v << 16);
        phi = dihedral4(P + 3 * k, P + 3 * u, P + 3 * v, P + 3 * l);
      }
    }
    ok = __all(good) != 0;
    if (!ok) return false;
    float cx = 0.f, cy = 0.f, cz = 0.f;
#pragma unroll
    for (int s = 0; s < TM_SLOTS; ++s) {
      const int a = lane + 64 * s;
      if (a < nl) {
        px[s] = P[3 * a]; py[s] = P[3 * a + 1]; pz[s] = P[3 * a + 2];
        tx[s] = T[3 * a]; ty[s] = T[3 * a + 1]; tz[s] = T[3 * a + 2];
        cx += tx[s]; cy += ty[s]; cz += tz[s];
        unsigned m = 0u;
        for (int r = 0; r < R; ++r) m |= (M[(size_t)r * mp.max_nl + a] ? 1u : 0u) << r;
        rot[s] = m;
      }
    }
    cx = wave_sum(cx) / (float)nl; cy = wave_sum(cy) / (float)nl; cz = wave_sum(cz) / (float)nl;
    double b2 = 0.0;
#pragma unroll
    for (int s = 0; s < TM_SLOTS; ++s) {
      if (lane + 64 * s < nl) {
        tx[s] -= cx; ty[s] -= cy; tz[s] -= cz;
        b2 += (double)tx[s] * tx[s] + (double)ty[s] * ty[s] + (double)tz[s] * tz[s];
      }
    }
    tb2 = wave_sum_d(b2);
    return true;
  }

  // f(theta); `theta` = theta_r on lane r < R
  CBD_DEV float eval(float theta) const {
    const int lane = lane_id();
    float x[TM_SLOTS], y[TM_SLOTS], z[TM_SLOTS];
#pragma unroll
    for (int s = 0; s < TM_SLOTS; ++s) { x[s] = px[s]; y[s] = py[s]; z[s] = pz[s]; }
    const float delta = lane < R ? sgn * (theta - phi) : 0.f;
    for (int r = 0; r < R; ++r) {
      const float th = __shfl(delta, r);
      const int q = __shfl(uv, r);
      const int u = q & 0xffff, v = q >> 16;
      const float ux = __shfl(slot_pick(x, u >> 6), u & 63), uy = __shfl(slot_pick(y, u >> 6), u & 63), uz = __shfl(slot_pick(z, u >> 6), u & 63);
      const float vx = __shfl(slot_pick(x, v >> 6), v & 63), vy = __shfl(slot_pick(y, v >> 6), v & 63), vz = __shfl(slot_pick(z, v >> 6), v & 63);
      float ax = ux - vx, ay = uy - vy, az = uz - vz;
      const float n = sqrtf(ax * ax + ay * ay + az * az);
      ax = ax / n * th; ay = ay / n * th; az = az / n * th;
      float Q[9];
      axis_angle_to_matrix(ax, ay, az, Q);
#pragma unroll
      for (int s = 0; s < TM_SLOTS; ++s) {
        if ((rot[s] >> r) & 1u) {
          const float dx = x[s] - vx, dy = y[s] - vy, dz = z[s] - vz;
          x[s] = Q[0] * dx + Q[1] * dy + Q[2] * dz + vx;
          y[s] = Q[3] * dx + Q[4] * dy + Q[5] * dz + vy;
          z[s] = Q[6] * dx + Q[7] * dy + Q[8] * dz + vz;
        }
      }
    }
    float cx = 0.f, cy = 0.f, cz = 0.f;
#pragma unroll
    for (int s = 0; s < TM_SLOTS; ++s)
      if (lane + 64 * s < nl) { cx += x[s]; cy += y[s]; cz += z[s]; }
    cx = wave_sum(cx) / (float)nl; cy = wave_sum(cy) / (float)nl; cz = wave_sum(cz) / (float)nl;
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double a2 = 0.0;
#pragma unroll
    for (int s = 0; s < TM_SLOTS; ++s) {
      if (lane + 64 * s < nl) {
        const double am[3] = {(double)(x[s] - cx), (double)(y[s] - cy), (double)(z[s] - cz)};
        const double bm[3] = {(double)tx[s], (double)ty[s], (double)tz[s]};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          a2 += am[i] * am[i];
#pragma unroll
          for (int k = 0; k < 3; ++k) S[3 * i + k] += am[i] * bm[k];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) S[i] = wave_sum_d(S[i]);
    a2 = wave_sum_d(a2);
    const double lam = horn_lambda_max(S);
    const double r2 = (a2 + tb2 - 2.0 * lam) / (double)nl;
    return (float)sqrt(fmax(r2, 0.0));
  }
};

// grid: n_problems * ceil(n_theta / 4) workgroups of 4 waves; wave w of workgroup g scores theta (g % per) * 4 + w of problem g / per
__global__ __launch_bounds__(64 * TM_WAVES) void match_score_kernel(MatchProblems mp, int n_theta, const float* __restrict__ theta,
                                                                    float* __restrict__ out) {
  const int per = (n_theta + TM_WAVES - 1) / TM_WAVES;
  const int p = blockIdx.x / per, t = (blockIdx.x % per) * TM_WAVES + (threadIdx.x >> 6);
  if (p >= mp.n || t >= n_theta) return;
  const int lane = lane_id();
  WaveProblem wp;
  const bool ok = wp.load(mp, p);
  float f = __builtin_nanf("");
  if (ok) {
    const float th = lane < wp.R ? theta[((size_t)p * n_theta + t) * mp.max_r + lane] : 0.f;
    f = wp.eval(th);
  }
  if (lane == 0) out[(size_t)p * n_theta + t] = f;
}

// ---- counter-based random numbers ----------------------------------------------------------------------------------------------------
enum : unsigned { RP_INIT = 1, RP_PERM = 2, RP_DITHER = 3, RP_PICK0 = 4, RP_PICK1 = 5, RP_FILL = 6, RP_CROSS = 7 };

CBD_DEV unsigned long long mix64(unsigned long long z) {   // splitmix64 finaliser
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// key: hash of (seed, problem id, generation)
CBD_DEV unsigned draw_u32(unsigned long long key, unsigned individual, unsigned dim, unsigned purpose) {
  return (unsigned)(mix64(key ^ (((unsigned long long)individual << 32) | (dim << 8) | purpose)) >> 32);
}
CBD_DEV float draw_unit(unsigned long long key, unsigned individual, unsigned dim, unsigned purpose) {   // [0, 1)
  return (float)(draw_u32(key, individual, dim, purpose) >> 8) * (1.0f / 16777216.0f);
}
// keyed permutation of [0, P): a bijection of [0, 2^bits) (add, odd multiply, xor-shift, all mod 2^bits), walked until it lands in [0, P)
CBD_DEV int keyed_perm(int i, int P, int bits, unsigned long long key, unsigned dim) {
  const unsigned m = (1u << bits) - 1u, sh = (unsigned)(bits + 1) >> 1;
  const unsigned k0 = draw_u32(key, 0, dim, RP_PERM), k1 = draw_u32(key, 1, dim, RP_PERM), k2 = draw_u32(key, 2, dim, RP_PERM);
  unsigned x = (unsigned)i;
  for (int guard = 0; guard <= (int)m; ++guard) {
    x = (x + k0) & m; x = (x * (k1 | 1u)) & m; x ^= x >> sh;
    x = (x + k2) & m; x = (x * ((k0 >> 7) | 1u)) & m; x ^= x >> sh;
    x = (x + (k1 >> 5)) & m; x = (x * ((k2 >> 3) | 1u)) & m; x ^= x >> sh;
    if (x < (unsigned)P) break;
  }
  return (int)x;
}
CBD_DEV float wrap_angle(float a) {   // into [-pi, pi)
  float w = a - 2.f * TM_PI * floorf((a + TM_PI) / (2.f * TM_PI));
  if (w >= TM_PI) w -= 2.f * TM_PI;
  return w < -TM_PI ? -TM_PI : w;
}

// fitness statistics by wave 0: best individual (lowest fitness, lowest index among equals), converged = std <= tol * |mean| (fp64,
// fixed order).  Results in s_stat[0] (best index) and s_stat[1] (converged).
CBD_DEV void de_stats(const float* fit, int P, float tol, int* s_stat) {
  const int lane = lane_id();
  unsigned long long best = ~0ull;
  double sum = 0.0;
  for (int i = lane; i < P; i += 64) {
    const float f = fit[i];
    const unsigned long long key = ((unsigned long long)__float_as_uint(f) << 32) | (unsigned)i;   // f >= 0: the bit pattern is monotone
    best = key < best ? key : best;
    sum += (double)f;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(best, o);
    best = w < best ? w : best;
  }
  const double mean = wave_sum_d(sum) / (double)P;
  double var = 0.0;
  for (int i = lane; i < P; i += 64) {
    const double d = (double)fit[i] - mean;
    var += d * d;
  }
  var = wave_sum_d(var) / (double)P;
  if (lane == 0) {
    s_stat[0] = (int)(best & 0xffffffffu);
    s_stat[1] = sqrt(var) <= (double)tol * fabs(mean) ? 1 : 0;
  }
}

// One workgroup per problem.  Dynamic LDS: pop [P][R], trial [P][R], fit [P], tfit [P] with P, R the launch's largest.
__global__ __launch_bounds__(64 * TM_WAVES) void match_de_kernel(MatchProblems mp, DeParams dp) {
  extern __shared__ float lds[];
  __shared__ int s_stat[2];
  const int p = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  WaveProblem wp;
  const bool ok = wp.load(mp, p);   // every wave loads the same description: uniform over the workgroup
  const int R = wp.R;
  const int P = max(dp.popsize * R, TM_MIN_POP);
  if (!ok || P > TM_MAX_POP) {
    if (tid == 0) { dp.fitness_out[p] = __builtin_nanf(""); dp.gens_out[p] = -1; }
    if (tid < mp.max_r) dp.theta_out[(size_t)p * mp.max_r + tid] = __builtin_nanf("");
    return;
  }
  const int cap = max(dp.popsize * mp.max_r, TM_MIN_POP) * mp.max_r;   // floats per population buffer (host sized the LDS with it)
  float* pop = lds;
  float* trial = lds + cap;
  float* fit = lds + 2 * cap;
  float* tfit = fit + TM_MAX_POP;
  const int PR = P * R;
  const unsigned long long key_p = mix64(mix64(dp.seed) ^ (unsigned long long)(unsigned)(dp.problem_id ? dp.problem_id[p] : p));
  int bits = 1;
  while ((1 << bits) < P) ++bits;
  // Latin hypercube: dimension j visits each of the P strata of [-pi, pi) once, in a keyed random order
  {
    const unsigned long long key = mix64(key_p);   // generation 0
    for (int idx = tid; idx < PR; idx += 64 * TM_WAVES) {
      const int i = idx / R, j = idx - i * R;
      const float u = draw_unit(key, i, j, RP_INIT);
      const float v = -TM_PI + 2.f * TM_PI * (((float)keyed_perm(i, P, bits, key, j) + u) / (float)P);
      pop[idx] = v >= TM_PI ? -TM_PI : v;
    }
  }
  __syncthreads();
  for (int i = wave; i < P; i += TM_WAVES) {
    const float f = wp.eval(lane < R ? pop[i * R + lane] : 0.f);
    if (lane == 0) fit[i] = f;
  }
  __syncthreads();
  if (wave == 0) de_stats(fit, P, dp.tol, s_stat);
  __syncthreads();
  int gens = 0;
  for (int gen = 1; gen <= dp.maxiter; ++gen) {
    const unsigned long long key = mix64(key_p ^ (unsigned long long)gen);
    const float F = dp.mut_lo + (dp.mut_hi - dp.mut_lo) * draw_unit(key, 0, 0, RP_DITHER);
    const int bi = s_stat[0];
    // best1bin: best + F (x_r0 - x_r1), r0 != r1 both != i; binomial crossover with one forced dimension
    for (int idx = tid; idx < PR; idx += 64 * TM_WAVES) {
      const int i = idx / R, j = idx - i * R;
      int r0 = (int)(draw_u32(key, i, 0, RP_PICK0) % (unsigned)(P - 1));
      if (r0 >= i) ++r0;
      int r1 = (int)(draw_u32(key, i, 0, RP_PICK1) % (unsigned)(P - 2));
      const int lo = min(i, r0), hi = max(i, r0);
      if (r1 >= lo) ++r1;
      if (r1 >= hi) ++r1;
      const int fill = (int)(draw_u32(key, i, 0, RP_FILL) % (unsigned)R);
      const bool cross = j == fill || draw_unit(key, i, j, RP_CROSS) < dp.recombination;
      // a mutant outside the bounds is wrapped periodically (the variable is an angle), not re-drawn
      trial[idx] = cross ? wrap_angle(pop[bi * R + j] + F * (pop[r0 * R + j] - pop[r1 * R + j])) : pop[idx];
    }
    __syncthreads();
    for (int i = wave; i < P; i += TM_WAVES) {
      const float f = wp.eval(lane < R ? trial[i * R + lane] : 0.f);
      if (lane == 0) tfit[i] = f;
    }
    __syncthreads();
    for (int idx = tid; idx < PR; idx += 64 * TM_WAVES) {   // greedy replacement, all at once
      const int i = idx / R;
      if (tfit[i] < fit[i]) pop[idx] = trial[idx];
    }
    __syncthreads();
    for (int i = tid; i < P; i += 64 * TM_WAVES)
      if (tfit[i] < fit[i]) fit[i] = tfit[i];
    __syncthreads();
    if (wave == 0) de_stats(fit, P, dp.tol, s_stat);
    __syncthreads();
    gens = gen;
    if (s_stat[1]) break;
  }
  const int bi = s_stat[0];
  if (tid < mp.max_r) dp.theta_out[(size_t)p * mp.max_r + tid] = tid < R ? pop[bi * R + tid] : 0.f;
  if (tid == 0) { dp.fitness_out[p] = fit[bi]; dp.gens_out[p] = gens; }
}

static size_t de_lds_bytes(int popsize, int max_r) {
  return ((size_t)2 * std::max(popsize * max_r, TM_MIN_POP) * max_r + 2 * TM_MAX_POP) * sizeof(float);
}
// the largest request the limits admit: 2 x 512 x 32 floats + 2 x 512 floats = 135168 B of the CU's 160 KiB
constexpr size_t TM_LDS_MAX = ((size_t)2 * TM_MAX_POP * TM_MAX_R + 2 * TM_MAX_POP) * sizeof(float);

}  // namespace cbd

using namespace cbd;

static int check_problems(int32_t n, int32_t max_nl, int32_t max_r, const void* probe, const void* target, const void* quads, const void* mask) {
  if (n < 0) return fail(CBD_ERR_ARG, "n_problems = %d", n);
  if (max_nl < 1 || max_nl > TM_MAX_NL) return fail(CBD_ERR_ARG, "Nl = %d outside 1..%d", max_nl, TM_MAX_NL);
  if (max_r < 1 || max_r > TM_MAX_R) return fail(CBD_ERR_ARG, "R = %d outside 1..%d (R = 0 needs no launch: align on the host)", max_r, TM_MAX_R);
  if (n > 0 && (!probe || !target || !quads || !mask)) return fail(CBD_ERR_ARG, "null problem description");
  return 0;
}

int cbd_match_score(int32_t n_problems, int32_t max_nl, int32_t max_r, int32_t n_theta, const int32_t* nl_dev, const int32_t* r_dev,
                    const float* probe_dev, const float* target_dev, const int32_t* quads_dev, const uint8_t* mask_rotate_dev,
                    const float* theta_dev, float* score_out_dev, void* stream) {
  CHK(check_problems(n_problems, max_nl, max_r, probe_dev, target_dev, quads_dev, mask_rotate_dev));
  if (n_theta < 0 || (n_problems > 0 && n_theta > 0 && (!theta_dev || !score_out_dev))) return fail(CBD_ERR_ARG, "bad argument");
  if (n_problems == 0 || n_theta == 0) return 0;
  const long long blocks = (long long)n_problems * ((n_theta + TM_WAVES - 1) / TM_WAVES);
  if (blocks > 0x7fffffffLL) return fail(CBD_ERR_ARG, "too many (problem, theta) pairs for one launch");
  const MatchProblems mp{n_problems, max_nl, max_r, nl_dev, r_dev, probe_dev, target_dev, quads_dev, mask_rotate_dev};
  hipLaunchKernelGGL(match_score_kernel, dim3((unsigned)blocks), dim3(64 * TM_WAVES), 0, reinterpret_cast<hipStream_t>(stream), mp, n_theta,
                     theta_dev, score_out_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int cbd_match_torsions(int32_t n_problems, int32_t max_nl, int32_t max_r, const int32_t* nl_dev, const int32_t* r_dev, const float* probe_dev,
                       const float* target_dev, const int32_t* quads_dev, const uint8_t* mask_rotate_dev, const int32_t* problem_id_dev,
                       uint64_t seed, int32_t popsize, int32_t maxiter, float mutation_lo, float mutation_hi, float recombination, float tol,
                       float* theta_out_dev, float* fitness_out_dev, int32_t* generations_out_dev, void* stream) {
  CHK(check_problems(n_problems, max_nl, max_r, probe_dev, target_dev, quads_dev, mask_rotate_dev));
  if (popsize < 1 || (long long)popsize * max_r > TM_MAX_POP)
    return fail(CBD_ERR_ARG, "popsize * R = %lld outside 1..%d", (long long)popsize * max_r, TM_MAX_POP);
  if (maxiter < 0 || !(mutation_lo >= 0.f) || !(mutation_hi >= mutation_lo) || !(mutation_hi < 2.f) || !(recombination >= 0.f) ||
      !(recombination <= 1.f) || !(tol >= 0.f))
    return fail(CBD_ERR_ARG, "bad differential-evolution parameter");
  if (n_problems > 0 && (!theta_out_dev || !fitness_out_dev || !generations_out_dev)) return fail(CBD_ERR_ARG, "null output");
  if (n_problems == 0) return 0;
  // the opt-in LDS size is a per-device function attribute
  static std::atomic<unsigned long long> attr_set{0};
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  const unsigned long long bit = 1ull << (dev & 63);
  if (!(attr_set.load(std::memory_order_acquire) & bit)) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&match_de_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TM_LDS_MAX));
    attr_set.fetch_or(bit, std::memory_order_release);
  }
  const MatchProblems mp{n_problems, max_nl, max_r, nl_dev, r_dev, probe_dev, target_dev, quads_dev, mask_rotate_dev};
  const DeParams dp{problem_id_dev, (unsigned long long)seed, popsize, maxiter, mutation_lo, mutation_hi, recombination, tol,
                    theta_out_dev, fitness_out_dev, generations_out_dev};
  hipLaunchKernelGGL(match_de_kernel, dim3(n_problems), dim3(64 * TM_WAVES), de_lds_bytes(popsize, max_r), reinterpret_cast<hipStream_t>(stream),
                     mp, dp);
  HIPCHK(hipGetLastError());
  return 0;
}
