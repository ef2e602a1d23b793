/* Exact k nearest neighbours on the CPU, for the tests of KDTreeMatcher knn = k (tests/test_knn_matcher.py).
 *
 * Arithmetic of the device (csrc/lsgpu_common.hip.h): dx = q - p in float, d2 = fmaf(dz,dz, fmaf(dy,dy, dx*dx)).
 * Every query's k matches in ascending (d2, reference index).  The reference is sorted by x once; a query sweeps outward
 * from its own x in both directions until fl(dx*dx) exceeds its current k-th distance -- exact, because d2 >= fl(dx*dx)
 * for every point further along (rounding is monotone and the fused terms are non-negative).
 * Build: cc -O2 -ffp-contract=off -fPIC -shared -pthread knn_brute.c -lm */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>

#define KNN_BRUTE_MAX_K 16

typedef struct { float x; int32_t i; } xkey;

static int xkey_cmp(const void* a, const void* b) {
  const xkey* p = (const xkey*)a; const xkey* q = (const xkey*)b;
  if (p->x != q->x) return p->x < q->x ? -1 : 1;
  return p->i < q->i ? -1 : (p->i > q->i);
}

typedef struct {
  const float* ref; const xkey* order; int64_t nr;
  const float* q; int64_t q0, q1; int k;
  int32_t* ids; float* d2;
} job;

static void insert(float* D, int32_t* I, int k, float d, int32_t i) {
  if (!(d < D[k - 1] || (d == D[k - 1] && i < I[k - 1]))) return;
  int s = k - 1;
  while (s > 0 && (d < D[s - 1] || (d == D[s - 1] && i < I[s - 1]))) { D[s] = D[s - 1]; I[s] = I[s - 1]; --s; }
  D[s] = d; I[s] = i;
}

static float dist2(const float* q, const float* p) {
  const float dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

static void* run(void* arg) {
  const job* J = (const job*)arg;
  const int k = J->k;
  for (int64_t j = J->q0; j < J->q1; ++j) {
    const float* q = J->q + 4 * j;
    float D[KNN_BRUTE_MAX_K]; int32_t I[KNN_BRUTE_MAX_K];
    for (int s = 0; s < k; ++s) { D[s] = INFINITY; I[s] = INT32_MAX; }
    int64_t lo = 0, hi = J->nr;   /* first position with x >= q.x */
    while (lo < hi) { const int64_t m = (lo + hi) / 2; if (J->order[m].x < q[0]) lo = m + 1; else hi = m; }
    int64_t up = lo, dn = lo - 1;
    int up_on = up < J->nr, dn_on = dn >= 0;
    while (up_on || dn_on) {
      if (up_on) {
        const xkey e = J->order[up];
        const float dx = q[0] - e.x;
        if (dx * dx > D[k - 1]) up_on = 0;
        else { insert(D, I, k, dist2(q, J->ref + 4 * (int64_t)e.i), e.i); up_on = ++up < J->nr; }
      }
      if (dn_on) {
        const xkey e = J->order[dn];
        const float dx = q[0] - e.x;
        if (dx * dx > D[k - 1]) dn_on = 0;
        else { insert(D, I, k, dist2(q, J->ref + 4 * (int64_t)e.i), e.i); dn_on = --dn >= 0; }
      }
    }
    for (int s = 0; s < k; ++s) {
      J->ids[j * k + s] = I[s] == INT32_MAX ? -1 : I[s];
      J->d2[j * k + s] = D[s];
    }
  }
  return NULL;
}

/* ids / d2: nq x k, query major.  threads: 1..16.  Returns 0, or -1 for a bad argument. */
int knn_brute(const float* ref_xyz1, int64_t nr, const float* q_xyz1, int64_t nq, int k, int threads,
              int32_t* ids, float* d2) {
  if (k < 1 || k > KNN_BRUTE_MAX_K || nr < 0 || nq < 0) return -1;
  if (threads < 1) threads = 1;
  if (threads > 16) threads = 16;
  xkey* order = (xkey*)malloc(sizeof(xkey) * (size_t)(nr > 0 ? nr : 1));
  if (!order) return -1;
  for (int64_t i = 0; i < nr; ++i) { order[i].x = ref_xyz1[4 * i]; order[i].i = (int32_t)i; }
  qsort(order, (size_t)nr, sizeof(xkey), xkey_cmp);
  pthread_t th[16];
  job jobs[16];
  const int64_t per = (nq + threads - 1) / threads;
  for (int t = 0; t < threads; ++t) {
    job* J = &jobs[t];
    J->ref = ref_xyz1; J->order = order; J->nr = nr; J->q = q_xyz1; J->k = k; J->ids = ids; J->d2 = d2;
    J->q0 = per * t < nq ? per * t : nq;
    J->q1 = per * (t + 1) < nq ? per * (t + 1) : nq;
    pthread_create(&th[t], NULL, run, J);
  }
  for (int t = 0; t < threads; ++t) pthread_join(th[t], NULL);
  free(order);
  return 0;
}
