// Plan, workspace layout and state block of the k-means launches: shared by kmeans.hip (Lloyd) and seg_kmeans.hip (the
// mini-batch centre update reads the partials an iic_kmeans_assign left in the same workspace).
#pragma once

#define KM_ROWS 64
#define KM_THREADS 256
#define KM_MAXK 256
#define KM_MAXD 32768
#define KM_MAXM 64                       // tiles per workgroup: P <= 4096 rows
#define KM_GROUP 32                      // partials per first-level reduction group
#define KM_SEED_WGS 1024
#define KM_MAXCAND 8

struct km_state {
  int iter;          // completed Lloyd iterations
  int converged;     // 0 running, 1 labels unchanged, 2 shift <= tol
  int pause;         // an empty cluster waits for the host's relocation
  int changed;       // labels changed by the current iteration's assignment
  double shift;      // last squared centre shift
  double inertia;    // sum of mind of the last assignment
  double tol;        // scaled tolerance (written by the host)
  double pad;
};

struct km_plan {
  int kb;            // 16-column blocks, a power of two
  int m;             // tiles per workgroup
  long W;            // workgroups = partials
  long W2;           // first-level groups (0: one level)
};

static bool km_plan_make(long n, int d, int k, km_plan* p) {
  if (n < 1 || n >= (1L << 31) || d < 1 || d > KM_MAXD || k < 1 || k > KM_MAXK) return false;
  int kb = 1;
  while (kb * 16 < k) kb *= 2;
  const long ntiles = (n + KM_ROWS - 1) / KM_ROWS;
  long m = kb * 4;                       // partial volume <= 1/16 of X: P = 16 * (padded k)
  const long fill = ntiles / 512 > 1 ? ntiles / 512 : 1;      // ... but at least ~512 workgroups when n allows
  if (m > fill) m = fill;
  if (m > KM_MAXM) m = KM_MAXM;
  p->kb = kb;
  p->m = (int)m;
  p->W = (ntiles + m - 1) / m;
  p->W2 = p->W > KM_GROUP ? (p->W + KM_GROUP - 1) / KM_GROUP : 0;
  return true;
}

// workspace layout, every region 256-byte aligned
struct km_ws {
  float* cnorm;              // [256]
  double* shift_part;        // [256]
  double* inertia_part;      // [W]
  int* count_part;           // [W][k]
  float* sum_part;           // [W][k][d]
  float* sum_part2;          // [W2][k][d]
  double* seed_part;         // [KM_SEED_WGS][8]
  long bytes;
};
static km_ws km_ws_make(void* base, const km_plan& p, int d, int k) {
  km_ws w;
  long off = 0;
  char* b = (char*)base;
  auto take = [&](long bytes) { char* r = b + off; off += (bytes + 255) & ~255L; return r; };
  w.cnorm = (float*)take(256 * 4);
  w.shift_part = (double*)take(256 * 8);
  w.inertia_part = (double*)take(p.W * 8);
  w.count_part = (int*)take(p.W * k * 4);
  w.sum_part = (float*)take(p.W * (long)k * d * 4);
  w.sum_part2 = (float*)take(p.W2 * (long)k * d * 4);
  w.seed_part = (double*)take((long)KM_SEED_WGS * KM_MAXCAND * 8);
  w.bytes = off;
  return w;
}
