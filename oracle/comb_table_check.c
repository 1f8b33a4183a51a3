/*
 * comb_table_check.c -- TEST INFRASTRUCTURE ONLY: an independent check of a run
 * of fixed-base comb table entries (the tables the verify kernels read; layout
 * in indy-plenum_amd/csrc/comb.h, restated here, none of its code used).
 *
 * Entry j of a row with base point R (= 2^(W*row) * P) holds (j+1) * R as an
 * affine niels point: 32 words = (y+x, y-x, 2dxy) as three field elements of ten
 * radix-2^25.5 limbs (even limbs 26 bits, odd limbs 25 bits) and 2 pad words.
 *
 * One call checks `count` consecutive entries.  For each entry:
 *   - every limb is in range and each field's value is below p (canonical),
 *   - words 30 and 31 are 0,
 *   - with x = (ypx - ymx) / 2 and y = (ypx + ymx) / 2, the third field is 2dxy,
 *   - the first entry is the expected point (given by the caller, computed with
 *     big integers),
 *   - every later entry is its predecessor plus the row base: the unified
 *     Edwards addition in projective form, compared by cross-multiplication
 *     (X3 = x Z3, Y3 = y Z3), so no inversion per entry.
 * The run is split over threads; each thread but the first starts from the
 * table's own entry just before its sub-range, which the previous thread's last
 * step verifies: when every thread reports no bad entry, induction from the
 * expected first point covers the whole run.  After a bad entry a thread goes on
 * from the point the entry should have held (one inversion), so one wrong entry
 * counts once; a sub-range whose starting entry turned out bad is checked again
 * from the corrected point once the threads have joined.
 *
 * The field arithmetic is the oracle's own (ed25519_oracle.c: radix 2^51,
 * 128-bit products), included below.
 */
#define _GNU_SOURCE
#include <pthread.h>

#include "ed25519_oracle.c"

#define CTC_ENTRY_WORDS 32
#define CTC_MAX_THREADS 256

/* ten limbs at bits 0, 26, 51, 77, ... -> radix 2^51; 0 when a limb is out of range or the value >= p */
static int limbs_to_fe(fe *r, const uint32_t *l) {
  int ok = 1;
  for (int i = 0; i < 5; i++) {
    ok &= l[2 * i] < (1u << 26) && l[2 * i + 1] < (1u << 25);
    r->v[i] = (uint64_t)l[2 * i] | ((uint64_t)l[2 * i + 1] << 26);
  }
  if (!ok) return 0;
  if (r->v[4] == M51 && r->v[3] == M51 && r->v[2] == M51 && r->v[1] == M51 && r->v[0] >= M51 - 18) return 0;
  return 1;
}

static int fe_equal(const fe *a, const fe *b) {
  fe d;
  fe_sub(&d, a, b);
  fe_canon(&d);
  return (d.v[0] | d.v[1] | d.v[2] | d.v[3] | d.v[4]) == 0;
}

typedef struct { fe x, y; } affine;

static fe C_half;

/* the entry's limb and pad checks, its point, and its third field; 1 when all hold */
static int entry_decode(affine *p, const uint32_t *e) {
  fe ypx, ymx, t, xy;
  int ok = limbs_to_fe(&ypx, e) & limbs_to_fe(&ymx, e + 10) & limbs_to_fe(&t, e + 20);
  ok &= e[30] == 0 && e[31] == 0;
  fe_sub(&p->x, &ypx, &ymx);
  fe_mul(&p->x, &p->x, &C_half);
  fe_add(&p->y, &ypx, &ymx);
  fe_mul(&p->y, &p->y, &C_half);
  fe_mul(&xy, &p->x, &p->y);
  fe_mul(&xy, &xy, &C_2d);
  return ok & fe_equal(&xy, &t);
}

typedef struct {
  const uint32_t *entries;
  uint64_t lo, hi;
  affine base, first;
  int have_first; /* thread 0: `first` is entry lo's expected point; others: start from entry lo - 1 */
  uint64_t bad, first_bad;
  affine end;   /* the point entry hi - 1 must hold (the entry's own when it passed) */
  int last_bad; /* entry hi - 1 failed */
} ctc_job;

static void *ctc_worker(void *arg) {
  ctc_job *j = (ctc_job *)arg;
  ge B, P, Q;
  affine prev, cur;
  B.X = j->base.x; B.Y = j->base.y; fe_1(&B.Z); fe_mul(&B.T, &B.X, &B.Y);
  j->bad = 0;
  j->first_bad = j->hi;
  j->last_bad = 0;
  if (!j->have_first) (void)entry_decode(&prev, j->entries + (j->lo - 1) * CTC_ENTRY_WORDS);
  for (uint64_t k = j->lo; k < j->hi; k++) {
    int ok = entry_decode(&cur, j->entries + k * CTC_ENTRY_WORDS);
    int stepped = !(k == j->lo && j->have_first);
    if (stepped) {
      fe l, r;
      P.X = prev.x; P.Y = prev.y; fe_1(&P.Z); fe_mul(&P.T, &P.X, &P.Y);
      ge_add(&Q, &P, &B);
      fe_mul(&l, &cur.x, &Q.Z);
      ok &= fe_equal(&l, &Q.X);
      fe_mul(&r, &cur.y, &Q.Z);
      ok &= fe_equal(&r, &Q.Y);
      fe_0(&l);
      ok &= !fe_equal(&Q.Z, &l); /* Z3 = 0 would make both compares hold */
    } else {
      ok &= fe_equal(&cur.x, &j->first.x) & fe_equal(&cur.y, &j->first.y);
    }
    j->last_bad = !ok;
    if (ok) {
      prev = cur;
    } else {
      if (!j->bad) j->first_bad = k;
      j->bad++;
      if (stepped) { /* go on from the point this entry should hold */
        fe zi;
        fe_invert(&zi, &Q.Z);
        fe_mul(&prev.x, &Q.X, &zi);
        fe_mul(&prev.y, &Q.Y, &zi);
      } else {
        prev = j->first;
      }
    }
  }
  j->end = prev;
  return NULL;
}

/* entries: count * 32 words.  base_xy / first_xy: x then y, 32-byte little-endian integers below p
 * (the row base, and the point entries[0] must hold).  Returns the number of bad entries and writes
 * the index of the first to *first_bad (count when there is none); -1 on a bad argument. */
int64_t comb_table_check(const uint32_t *entries, uint64_t count, const uint8_t base_xy[64],
                         const uint8_t first_xy[64], int threads, uint64_t *first_bad) {
  if (!entries || !base_xy || !first_xy || !first_bad || threads < 1) return -1;
  if (threads > CTC_MAX_THREADS) threads = CTC_MAX_THREADS;
  if ((uint64_t)threads > count) threads = count ? (int)count : 1;
  init_consts();
  fe two;
  fe_0(&two);
  two.v[0] = 2;
  fe_invert(&C_half, &two);
  ctc_job job[CTC_MAX_THREADS];
  pthread_t tid[CTC_MAX_THREADS];
  int started = 0;
  for (int t = 0; t < threads; t++) {
    ctc_job *j = &job[t];
    j->entries = entries;
    j->lo = count * (uint64_t)t / (uint64_t)threads;
    j->hi = count * (uint64_t)(t + 1) / (uint64_t)threads;
    fe_frombytes(&j->base.x, base_xy);
    fe_frombytes(&j->base.y, base_xy + 32);
    fe_frombytes(&j->first.x, first_xy);
    fe_frombytes(&j->first.y, first_xy + 32);
    j->have_first = t == 0;
    if (threads == 1) {
      ctc_worker(j);
    } else {
      if (pthread_create(&tid[t], NULL, ctc_worker, j) != 0) break;
      started++;
    }
  }
  for (int t = 0; t < started; t++) pthread_join(tid[t], NULL);
  if (threads > 1 && started != threads) return -1;
  for (int t = 1; t < threads; t++) { /* a sub-range that started from a bad entry: again, from the right point */
    if (!job[t - 1].last_bad || job[t].lo == job[t].hi) continue;
    ge B, P, Q;
    fe zi;
    B.X = job[t].base.x; B.Y = job[t].base.y; fe_1(&B.Z); fe_mul(&B.T, &B.X, &B.Y);
    P.X = job[t - 1].end.x; P.Y = job[t - 1].end.y; fe_1(&P.Z); fe_mul(&P.T, &P.X, &P.Y);
    ge_add(&Q, &P, &B);
    fe_invert(&zi, &Q.Z);
    fe_mul(&job[t].first.x, &Q.X, &zi);
    fe_mul(&job[t].first.y, &Q.Y, &zi);
    job[t].have_first = 1;
    ctc_worker(&job[t]);
  }
  uint64_t bad = 0;
  *first_bad = count;
  for (int t = 0; t < threads; t++) {
    if (job[t].bad && *first_bad == count) *first_bad = job[t].first_bad;
    bad += job[t].bad;
  }
  return (int64_t)bad;
}
