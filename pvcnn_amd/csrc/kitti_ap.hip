// kitti_ap.hip -- the KITTI AP evaluation (evaluate/kitti/utils/eval.py: image_box_overlap, clean_data, compute_statistics_jit,
// get_thresholds, fused_compute_statistics) on the device.
//
// The reference runs one sequential greedy matching per (image, score threshold, class, difficulty, min_overlap row) in numba loops.
// Here a matching is the work of ONE WAVE: the ground truths of the image are visited in order (the matching is sequential in them),
// the detections lie across the lanes (detection j belongs to lane j & 63, round j >> 6), and the choice of a ground truth's detection
// is a wave reduction.  What the reference keeps per detection (assigned_detection, ignored_threshold) is ONE BIT per detection in
// 32-bit lane registers -- bit t of lane l is detection 64 t + l -- hence the limit of 2048 detections per image (PVCNN_KITTI_AP_MAX_BOXES).
//
// All data is ragged per image, described by prefix offsets: gt_off, dt_off, dc_off (I + 1) and pair_off (image i holds dt_i x gt_i
// overlaps, overlaps[pair_off[i] + det * gt_i + gt]).  A "cell" is (class m, difficulty l, min_overlap row k), index (m * L + l) * K + k;
// its min_overlap is min_overlaps[k * M + m] (the reference's min_overlaps[:, metric, m]).
//
// Nothing here uses an atomic, and every sum is taken in an order fixed by the sizes alone: two runs give the same bits.
#include <climits>

#include "wave.h"

namespace pvcnn {

constexpr int kApThreads = 256;
constexpr int kApWaves = kApThreads / kWave;
constexpr int kApImagesPerWave = 8;                 // images a wave matches one after the other (a KITTI image has ~10 boxes)
constexpr int kApSlots = PVCNN_KITTI_AP_SAMPLE_POINTS;
constexpr int kApMaxBoxes = PVCNN_KITTI_AP_MAX_BOXES;
constexpr double kNoDetection = -10000000.0;        // compute_statistics_jit's _no_detection: no score at or below it is ever matched
static_assert(kApMaxBoxes == 32 * kWave, "one bit per detection in a 32-bit lane register");

// image_box_overlap for one pair, the reference's expression with one rounding per operation (never contracted: a fused
// a*b + c - d*e changes the last bit)
__device__ __forceinline__ double image_overlap(const double *__restrict__ b, const double *__restrict__ q, int criterion) {
#pragma clang fp contract(off)
  const double qbox_area = (q[2] - q[0]) * (q[3] - q[1]);
  const double iw = fmin(b[2], q[2]) - fmax(b[0], q[0]);
  if (!(iw > 0.0)) return 0.0;
  const double ih = fmin(b[3], q[3]) - fmax(b[1], q[1]);
  if (!(ih > 0.0)) return 0.0;
  double ua;
  if (criterion == -1) {
    ua = (b[2] - b[0]) * (b[3] - b[1]) + qbox_area - iw * ih;
  } else if (criterion == 0) {
    ua = (b[2] - b[0]) * (b[3] - b[1]);
  } else if (criterion == 1) {
    ua = qbox_area;
  } else {
    ua = 1.0;
  }
  return iw * ih / ua;
}

__global__ __launch_bounds__(kApThreads) void image_box_overlap_kernel(const double *__restrict__ boxes, long long N,
                                                                      const double *__restrict__ query, long long K, int criterion,
                                                                      double *__restrict__ out) {
  const long long p = (long long)blockIdx.x * kApThreads + threadIdx.x;
  if (p >= N * K) return;
  out[p] = image_overlap(boxes + 4 * (p / K), query + 4 * (p % K), criterion);
}

// per-image blocks: boxes = detections, query boxes = ground truths
__global__ __launch_bounds__(kApThreads) void bbox_overlaps_kernel(const double *__restrict__ dt_bbox, const double *__restrict__ gt_bbox,
                                                                  const long long *__restrict__ dt_off, const long long *__restrict__ gt_off,
                                                                  const long long *__restrict__ pair_off, long long images, long long total,
                                                                  double *__restrict__ out) {
  const long long p = (long long)blockIdx.x * kApThreads + threadIdx.x;
  if (p >= total) return;
  long long lo = 0, hi = images;                       // the last image with pair_off[i] <= p
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (pair_off[mid] <= p) lo = mid; else hi = mid;
  }
  const long long nd = dt_off[lo + 1] - dt_off[lo], ng = gt_off[lo + 1] - gt_off[lo], r = p - pair_off[lo];
  if (ng <= 0 || r >= nd * ng) return;
  out[p] = image_overlap(dt_bbox + 4 * (dt_off[lo] + r / ng), gt_bbox + 4 * (gt_off[lo] + r % ng), -1);
}

// ---- clean_data for every (class, difficulty) ---------------------------------------------------------------------------------------
// names are codes: 0 car, 1 pedestrian, 2 cyclist, 3 van, 4 person_sitting, 6 tractor, 7 trailer (lower-cased match), -2 the exact
// string 'DontCare', -1 anything else.  Class 5 of the reference's table is 'car' again.
__device__ __forceinline__ int class_code(int current_class) { return current_class == 5 ? 0 : current_class; }

__device__ __forceinline__ void difficulty_limits(int difficulty, double &min_height, double &max_occlusion, double &max_truncation) {
  min_height = difficulty == 0 ? 40.0 : 25.0;
  max_occlusion = (double)difficulty;
  max_truncation = difficulty == 0 ? 0.15 : difficulty == 1 ? 0.3 : 0.5;
}

__global__ __launch_bounds__(kApThreads) void clean_kernel(const int *__restrict__ gt_name, const double *__restrict__ gt_bbox,
                                                          const double *__restrict__ gt_occluded, const double *__restrict__ gt_truncated,
                                                          long long G, const int *__restrict__ dt_name, const double *__restrict__ dt_bbox,
                                                          long long D, const int *__restrict__ classes, const int *__restrict__ difficulties,
                                                          int L, signed char *__restrict__ ignored_gt, signed char *__restrict__ ignored_det) {
  const int cd = blockIdx.y, code = class_code(classes[cd / L]);
  double min_height, max_occlusion, max_truncation;
  difficulty_limits(difficulties[cd % L], min_height, max_occlusion, max_truncation);
  const long long i = (long long)blockIdx.x * kApThreads + threadIdx.x;
  if (i < G) {
    const int name = gt_name[i];
    const double height = gt_bbox[4 * i + 3] - gt_bbox[4 * i + 1];
    const int valid_class = name == code ? 1 : (code == 1 && name == 4) || (code == 0 && name == 3) ? 0 : -1;
    const bool ignore = gt_occluded[i] > max_occlusion || gt_truncated[i] > max_truncation || height <= min_height;
    ignored_gt[cd * G + i] = (valid_class == 1 && !ignore) ? 0 : (valid_class == 0 || (ignore && valid_class == 1)) ? 1 : -1;
  }
  if (i < D) {
    const double height = fabs(dt_bbox[4 * i + 3] - dt_bbox[4 * i + 1]);
    ignored_det[cd * D + i] = height < min_height ? 1 : dt_name[i] == code ? 0 : -1;
  }
}

// num_valid_gt[cd] = #(ignored_gt[cd] == 0): one workgroup per (class, difficulty), integer sums
__global__ __launch_bounds__(kApThreads) void count_valid_kernel(const signed char *__restrict__ ignored_gt, long long G,
                                                                long long *__restrict__ num_valid_gt) {
  __shared__ long long red[kApThreads];
  const signed char *row = ignored_gt + (long long)blockIdx.x * G;
  long long n = 0;
  for (long long i = threadIdx.x; i < G; i += kApThreads) n += row[i] == 0 ? 1 : 0;
  red[threadIdx.x] = n;
  __syncthreads();
  for (int w = kApThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) num_valid_gt[blockIdx.x] = red[0];
}

// the DontCare ground truths of every image, in order: dc_index[dc_off[i] ..] = their positions in the flat ground-truth arrays
__global__ __launch_bounds__(kApThreads) void dontcare_kernel(const int *__restrict__ gt_name, const long long *__restrict__ gt_off,
                                                             const long long *__restrict__ dc_off, long long images,
                                                             int *__restrict__ dc_index) {
  const long long i = (long long)blockIdx.x * kApThreads + threadIdx.x;
  if (i >= images) return;
  long long at = dc_off[i];
  const long long end = dc_off[i + 1];
  for (long long g = gt_off[i]; g < gt_off[i + 1] && at < end; ++g)
    if (gt_name[g] == -2) dc_index[at++] = (int)g;
}

// ---- wave reductions: every lane ends with the same result ------------------------------------------------------------------------------
// the largest value; among equal values the lowest index
__device__ __forceinline__ void wave_best(double &v, int &j) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int oj = __shfl_xor(j, o);
    if (ov > v || (ov == v && oj < j)) {
      v = ov;
      j = oj;
    }
  }
}

struct ApData {
  const double *overlaps;                              // per-image (dt_i, gt_i) blocks at pair_off[i]
  const long long *gt_off, *dt_off, *dc_off, *pair_off;
  const signed char *ignored_gt, *ignored_det;         // (M * L, G), (M * L, D)
  const double *dt_score, *dt_alpha, *gt_alpha, *dt_bbox, *gt_bbox;
  const int *dc_index;
  const double *min_overlaps;                          // (K, M)
  long long images, G, D;
  int M, L, K;
};

// one image of a wave: its sizes, clipped to what the lane registers hold (the entry points refuse larger images)
struct ApImage {
  long long g0, d0, pairs;
  int ng, nd, rounds;
  const signed char *igt, *idt;
};
__device__ __forceinline__ ApImage ap_image(const ApData &a, long long i, int cd) {
  ApImage m;
  m.g0 = a.gt_off[i];
  m.d0 = a.dt_off[i];
  m.pairs = a.pair_off[i];
  m.ng = (int)min(a.gt_off[i + 1] - m.g0, (long long)kApMaxBoxes);
  m.nd = (int)min(a.dt_off[i + 1] - m.d0, (long long)kApMaxBoxes);
  m.rounds = (m.nd + kWave - 1) / kWave;
  m.igt = a.ignored_gt + cd * a.G + m.g0;
  m.idt = a.ignored_det + cd * a.D + m.d0;
  return m;
}

// ---- matching pass 1 (compute_fp = False): for each ground truth in order, the unassigned, non-(-1) detection with overlap >
// min_overlap and the highest score (lowest index among equals).  tp_scores (cells, G): the score of a true positive in the slot of
// its ground truth, -inf in every other slot.
__global__ __launch_bounds__(kApThreads) void match_kernel(ApData a, long long chunks, double *__restrict__ tp_scores) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long chunk = (long long)blockIdx.x * kApWaves + (threadIdx.x >> 6);
  if (chunk >= chunks) return;
  const int cell = blockIdx.y, cd = cell / a.K, k = cell % a.K;
  const double min_overlap = a.min_overlaps[k * a.M + cd / a.L];
  for (long long i = chunk * kApImagesPerWave; i < min(a.images, (chunk + 1) * kApImagesPerWave); ++i) {
    const ApImage m = ap_image(a, i, cd);
    double *slots = tp_scores + cell * a.G + m.g0;
    unsigned usable = 0u;                               // not ignored_det == -1 and not yet assigned
    for (int t = 0; t < m.rounds; ++t) {
      const int j = t * kWave + lane;
      if (j < m.nd && m.idt[j] != -1) usable |= 1u << t;
    }
    for (int g = 0; g < m.ng; ++g) {
      const int ig = m.igt[g];
      double tp_score = -INFINITY;
      if (ig != -1) {
        double best = kNoDetection;
        int det = INT_MAX;
        for (int t = 0; t < m.rounds; ++t) {
          if (!((usable >> t) & 1u)) continue;
          const int j = t * kWave + lane;
          const double score = a.dt_score[m.d0 + j];
          if (a.overlaps[m.pairs + (long long)j * m.ng + g] > min_overlap && score > best) {
            best = score;
            det = j;
          }
        }
        wave_best(best, det);
        if (det != INT_MAX) {
          if (lane == (det & (kWave - 1))) usable &= ~(1u << (det >> 6));
          if (!(ig == 1 || m.idt[det] == 1)) tp_score = best;
        }
      }
      if (lane == 0) slots[g] = tp_score;
    }
  }
}

// ---- get_thresholds on the descending scores of a cell (the -inf slots sort to the end): one wave per cell.  The reference walks
// the scores and `continue`s while (r_recall - current_recall) < (current_recall - l_recall); 64 scores are tested at once and the
// first that does not skip is taken.  current_recall is the same repeated fp64 addition of 1 / 40, the recalls the same divisions.
__global__ __launch_bounds__(kWave) void thresholds_kernel(const double *__restrict__ sorted, long long G,
                                                          const long long *__restrict__ num_valid_gt, int K,
                                                          double *__restrict__ thresholds, int *__restrict__ counts) {
  const int lane = threadIdx.x, cell = blockIdx.x;
  const double *scores = sorted + cell * G;
  int mine = 0;
  for (long long i = lane; i < G; i += kWave) mine += scores[i] > -INFINITY ? 1 : 0;
  const long long n = wave_sum(mine);
  const double num_gt = (double)num_valid_gt[cell / K];
  double current_recall = 0.0;
  int count = 0;
  long long i = 0;
  while (i < n && count < kApSlots) {
    const long long ii = i + lane;
    const double l_recall = (double)(ii + 1) / num_gt;
    const double r_recall = ii < n - 1 ? (double)(ii + 2) / num_gt : l_recall;
    const bool skip = (r_recall - current_recall) < (current_recall - l_recall) && ii < n - 1;
    const unsigned long long take = __ballot(ii < n && !skip);
    if (take == 0ull) {
      i += kWave;
      continue;
    }
    const long long at = i + (__ffsll((long long)take) - 1);
    if (lane == 0) thresholds[cell * kApSlots + count] = scores[at];
    ++count;
    current_recall += 1.0 / (kApSlots - 1.0);
    i = at + 1;
  }
  for (int s = count + lane; s < kApSlots; s += kWave) thresholds[cell * kApSlots + s] = 0.0;
  if (lane == 0) counts[cell] = count;
}

// ---- matching pass 2 (compute_fp = True) at the score threshold of slot blockIdx.y: tp, fp, fn and the orientation similarity of
// kApImagesPerWave images per wave, summed in image order into partial (cells, 41, chunks, 4).
// The reference's scan over the detections of a ground truth ends, whatever the order of the candidates (unassigned, score >=
// thresh, overlap > min_overlap >= 0), on: the ignored_det == 0 candidate with the largest overlap, the lowest index among equals
// (the first such candidate is always taken -- max_overlap is 0 or assigned_ignored_det is set -- and a later one replaces it only
// with a strictly larger overlap); without one, the FIRST ignored_det == 1 candidate (taken only while nothing is chosen).
__global__ __launch_bounds__(kApThreads) void stats_kernel(ApData a, long long chunks, const double *__restrict__ thresholds,
                                                          const int *__restrict__ counts, int metric, int compute_aos,
                                                          double *__restrict__ partial) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long chunk = (long long)blockIdx.x * kApWaves + (threadIdx.x >> 6);
  if (chunk >= chunks) return;
  const int slot = blockIdx.y, cell = blockIdx.z, cd = cell / a.K, k = cell % a.K;
  const double min_overlap = a.min_overlaps[k * a.M + cd / a.L];
  long long tp = 0, fp = 0, fn = 0;
  double similarity = 0.0;
  if (slot < counts[cell]) {
    const double thresh = thresholds[cell * kApSlots + slot];
    for (long long i = chunk * kApImagesPerWave; i < min(a.images, (chunk + 1) * kApImagesPerWave); ++i) {
      const ApImage m = ap_image(a, i, cd);
      unsigned usable = 0u, ignored = 0u;               // usable: not -1, not below the threshold, not yet assigned; ignored: == 1
      for (int t = 0; t < m.rounds; ++t) {
        const int j = t * kWave + lane;
        if (j >= m.nd) continue;
        const int c = m.idt[j];
        if (c != -1 && !(a.dt_score[m.d0 + j] < thresh)) usable |= 1u << t;
        if (c == 1) ignored |= 1u << t;
      }
      for (int g = 0; g < m.ng; ++g) {
        const int ig = m.igt[g];
        if (ig == -1) continue;
        double best = -INFINITY;
        int det = INT_MAX, first_ignored = INT_MAX;
        for (int t = 0; t < m.rounds; ++t) {
          if (!((usable >> t) & 1u)) continue;
          const int j = t * kWave + lane;
          const double overlap = a.overlaps[m.pairs + (long long)j * m.ng + g];
          if (!(overlap > min_overlap)) continue;
          if ((ignored >> t) & 1u) {
            if (first_ignored == INT_MAX) first_ignored = j;
          } else if (overlap > best) {
            best = overlap;
            det = j;
          }
        }
        wave_best(best, det);
        const bool chose_ignored = det == INT_MAX;
        if (chose_ignored) det = wave_min(first_ignored);
        if (det == INT_MAX) {
          fn += ig == 0 ? 1 : 0;
          continue;
        }
        if (lane == (det & (kWave - 1))) usable &= ~(1u << (det >> 6));
        if (ig == 1 || chose_ignored) continue;
        ++tp;
        if (compute_aos) similarity += (1.0 + cos(a.gt_alpha[m.g0 + g] - a.dt_alpha[m.d0 + det])) / 2.0;
      }
      // false positives: what is left of the ignored_det == 0 detections at or above the threshold; for the 2-D metric without
      // those that lie in a DontCare region (the "stuff" the reference subtracts)
      unsigned left = usable & ~ignored;
      if (metric == 0 && left != 0u) {
        const long long dc0 = a.dc_off[i], ndc = a.dc_off[i + 1] - dc0;
        for (int t = 0; t < m.rounds; ++t) {
          if (!((left >> t) & 1u)) continue;
          const double *box = a.dt_bbox + 4 * (m.d0 + t * kWave + lane);
          for (long long c = 0; c < ndc; ++c) {
            if (image_overlap(box, a.gt_bbox + 4ll * a.dc_index[dc0 + c], 0) > min_overlap) {
              left &= ~(1u << t);
              break;
            }
          }
        }
      }
      fp += wave_sum((int)__popc(left));
    }
  }
  if (lane == 0) {
    double *out = partial + (((long long)cell * kApSlots + slot) * chunks + chunk) * 4;
    out[0] = (double)tp;
    out[1] = (double)fp;
    out[2] = (double)fn;
    out[3] = similarity;
  }
}

// pr (cells, 41, 4) = the partials of a (cell, slot) summed in a fixed order: lane l takes chunks l, l + 64, .. in order, then a
// butterfly over the lanes.  tp / fp / fn are integers below 2^53 carried in fp64 (exact).
__global__ __launch_bounds__(kWave) void reduce_kernel(const double *__restrict__ partial, long long chunks, double *__restrict__ pr) {
  const int lane = threadIdx.x;
  const double *in = partial + (long long)blockIdx.x * chunks * 4;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long c = lane; c < chunks; c += kWave) {
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] += in[c * 4 + q];
  }
  s[0] = wave_sum(s[0]); s[1] = wave_sum(s[1]); s[2] = wave_sum(s[2]); s[3] = wave_sum(s[3]);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) pr[(long long)blockIdx.x * 4 + q] = s[q];
  }
}

static long long ap_chunks(long long images) { return (images + kApImagesPerWave - 1) / kApImagesPerWave; }

}  // namespace pvcnn

using namespace pvcnn;

extern "C" int pvcnn_image_box_overlap(const double *boxes, long long N, const double *query_boxes, long long K, int criterion,
                                       double *out, void *stream) {
  PVCNN_REQUIRE(N >= 0 && K >= 0, "bad sizes");
  if (N == 0 || K == 0) return 0;
  PVCNN_REQUIRE(boxes && query_boxes && out, "null pointer");
  PVCNN_REQUIRE(N <= (1ll << 38) / K, "N * K must be <= 2^38");
  hipLaunchKernelGGL(image_box_overlap_kernel, dim3((unsigned)((N * K + kApThreads - 1) / kApThreads)), dim3(kApThreads), 0,
                     static_cast<hipStream_t>(stream), boxes, N, query_boxes, K, criterion, out);
  return check_launch("image_box_overlap");
}

extern "C" int pvcnn_kitti_ap_bbox_overlaps(const double *dt_bbox, const double *gt_bbox, const long long *dt_off, const long long *gt_off,
                                            const long long *pair_off, long long images, long long total_pairs, double *out,
                                            void *stream) {
  PVCNN_REQUIRE(images >= 0 && total_pairs >= 0, "bad sizes");
  if (images == 0 || total_pairs == 0) return 0;
  PVCNN_REQUIRE(dt_bbox && gt_bbox && dt_off && gt_off && pair_off && out, "null pointer");
  const long long blocks = (total_pairs + kApThreads - 1) / kApThreads;
  PVCNN_REQUIRE(blocks < (1ll << 31), "too many pairs");
  hipLaunchKernelGGL(bbox_overlaps_kernel, dim3((unsigned)blocks), dim3(kApThreads), 0, static_cast<hipStream_t>(stream), dt_bbox, gt_bbox,
                     dt_off, gt_off, pair_off, images, total_pairs, out);
  return check_launch("kitti_ap_bbox_overlaps");
}

extern "C" int pvcnn_kitti_ap_clean(const int *gt_name, const double *gt_bbox, const double *gt_occluded, const double *gt_truncated,
                                    long long G, const int *dt_name, const double *dt_bbox, long long D, const long long *gt_off,
                                    const long long *dc_off, long long images, const int *classes, int num_classes, const int *difficulties,
                                    int num_difficulties, signed char *ignored_gt, signed char *ignored_det, int *dc_index,
                                    long long *num_valid_gt, void *stream) {
  PVCNN_REQUIRE(G >= 0 && D >= 0 && images >= 0 && G < (1ll << 31) && D < (1ll << 31), "bad sizes");
  PVCNN_REQUIRE(num_classes > 0 && num_difficulties > 0 && (long long)num_classes * num_difficulties <= 65535,
                "classes * difficulties must be in [1, 65535]");
  PVCNN_REQUIRE(classes && difficulties && num_valid_gt, "null pointer");
  PVCNN_REQUIRE(G == 0 || (gt_name && gt_bbox && gt_occluded && gt_truncated && ignored_gt), "null pointer");
  PVCNN_REQUIRE(D == 0 || (dt_name && dt_bbox && ignored_det), "null pointer");
  PVCNN_REQUIRE(images == 0 || (gt_off && dc_off), "null pointer");
  PVCNN_REQUIRE(G == 0 || images == 0 || dc_index, "null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int cells = num_classes * num_difficulties;
  const long long most = G > D ? G : D;
  if (most > 0) {
    hipLaunchKernelGGL(clean_kernel, dim3((unsigned)((most + kApThreads - 1) / kApThreads), (unsigned)cells), dim3(kApThreads), 0, s, gt_name,
                       gt_bbox, gt_occluded, gt_truncated, G, dt_name, dt_bbox, D, classes, difficulties, num_difficulties, ignored_gt,
                       ignored_det);
  }
  hipLaunchKernelGGL(count_valid_kernel, dim3((unsigned)cells), dim3(kApThreads), 0, s, ignored_gt, G, num_valid_gt);
  if (images > 0 && G > 0) {
    hipLaunchKernelGGL(dontcare_kernel, dim3((unsigned)((images + kApThreads - 1) / kApThreads)), dim3(kApThreads), 0, s, gt_name, gt_off,
                       dc_off, images, dc_index);
  }
  return check_launch("kitti_ap_clean");
}

static int ap_check(const ApData &a, int max_gt, int max_dt, const char **why) {
  *why = nullptr;
  if (a.images < 0 || a.G < 0 || a.D < 0 || a.M <= 0 || a.L <= 0 || a.K <= 0) *why = "bad sizes";
  else if ((long long)a.M * a.L * a.K > 65535) *why = "classes * difficulties * min_overlap rows must be <= 65535";
  else if (max_gt < 0 || max_dt < 0) *why = "bad per-image maxima";
  else if (max_gt > kApMaxBoxes) *why = "an image has more than 2048 ground truths (PVCNN_KITTI_AP_MAX_BOXES)";
  else if (max_dt > kApMaxBoxes) *why = "an image has more than 2048 detections (PVCNN_KITTI_AP_MAX_BOXES)";
  else if (ap_chunks(a.images) / kApWaves >= (1ll << 31)) *why = "too many images";
  else if (!a.min_overlaps) *why = "null pointer";
  else if (a.images > 0 && !(a.gt_off && a.dt_off && a.dc_off && a.pair_off)) *why = "null pointer";
  else if (a.G > 0 && !(a.ignored_gt && a.gt_alpha && a.gt_bbox)) *why = "null pointer";
  else if (a.D > 0 && !(a.ignored_det && a.dt_score && a.dt_alpha && a.dt_bbox)) *why = "null pointer";
  else if (a.G > 0 && a.D > 0 && max_gt > 0 && max_dt > 0 && !a.overlaps) *why = "null pointer";
  return *why ? PVCNN_ERR_INVALID_ARGUMENT : 0;
}

#define PVCNN_AP_ARGS                                                                                                                  \
  const double *overlaps, const long long *gt_off, const long long *dt_off, const long long *dc_off, const long long *pair_off,         \
      long long images, long long G, long long D, int max_gt, int max_dt, const signed char *ignored_gt, const signed char *ignored_det, \
      const double *dt_score, const double *dt_alpha, const double *gt_alpha, const double *dt_bbox, const double *gt_bbox,              \
      const int *dc_index, const double *min_overlaps, int num_classes, int num_difficulties, int num_min_overlaps
#define PVCNN_AP_DATA                                                                                                                   \
  ApData {                                                                                                                              \
    overlaps, gt_off, dt_off, dc_off, pair_off, ignored_gt, ignored_det, dt_score, dt_alpha, gt_alpha, dt_bbox, gt_bbox, dc_index,        \
        min_overlaps, images, G, D, num_classes, num_difficulties, num_min_overlaps                                                     \
  }

extern "C" int pvcnn_kitti_ap_match(PVCNN_AP_ARGS, double *tp_scores, void *stream) {
  const ApData a = PVCNN_AP_DATA;
  const char *why;
  if (ap_check(a, max_gt, max_dt, &why)) PVCNN_REQUIRE(false, why);
  if (a.images == 0 || a.G == 0) return 0;
  PVCNN_REQUIRE(tp_scores, "null pointer");
  const long long chunks = ap_chunks(a.images);
  hipLaunchKernelGGL(match_kernel, dim3((unsigned)((chunks + kApWaves - 1) / kApWaves), (unsigned)(a.M * a.L * a.K)), dim3(kApThreads), 0,
                     static_cast<hipStream_t>(stream), a, chunks, tp_scores);
  return check_launch("kitti_ap_match");
}

extern "C" int pvcnn_kitti_ap_thresholds(const double *sorted_scores, long long G, const long long *num_valid_gt, int num_cells,
                                         int num_min_overlaps, double *thresholds, int *counts, void *stream) {
  PVCNN_REQUIRE(G >= 0 && num_cells > 0 && num_min_overlaps > 0 && num_cells % num_min_overlaps == 0, "bad sizes");
  PVCNN_REQUIRE(num_valid_gt && thresholds && counts && (G == 0 || sorted_scores), "null pointer");
  hipLaunchKernelGGL(thresholds_kernel, dim3((unsigned)num_cells), dim3(kWave), 0, static_cast<hipStream_t>(stream), sorted_scores, G,
                     num_valid_gt, num_min_overlaps, thresholds, counts);
  return check_launch("kitti_ap_thresholds");
}

extern "C" size_t pvcnn_kitti_ap_workspace_bytes(long long images, int num_cells) {
  if (images <= 0 || num_cells <= 0) return 0;
  return (size_t)num_cells * kApSlots * (size_t)ap_chunks(images) * 4 * sizeof(double);
}

extern "C" int pvcnn_kitti_ap_stats(PVCNN_AP_ARGS, const double *thresholds, const int *counts, int metric, int compute_aos, double *pr,
                                    void *workspace, size_t workspace_bytes, void *stream) {
  const ApData a = PVCNN_AP_DATA;
  const char *why;
  if (ap_check(a, max_gt, max_dt, &why)) PVCNN_REQUIRE(false, why);
  PVCNN_REQUIRE(metric >= 0 && metric <= 2, "metric must be 0, 1 or 2");
  PVCNN_REQUIRE(thresholds && counts && pr, "null pointer");
  PVCNN_REQUIRE(a.G == 0 || metric != 0 || a.dc_index, "null pointer");
  const int cells = a.M * a.L * a.K;
  const long long chunks = ap_chunks(a.images);
  PVCNN_REQUIRE(a.images == 0 || (workspace && workspace_bytes >= pvcnn_kitti_ap_workspace_bytes(a.images, cells)), "workspace too small");
  PVCNN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "workspace must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  double *partial = static_cast<double *>(workspace);
  if (chunks > 0) {
    hipLaunchKernelGGL(stats_kernel, dim3((unsigned)((chunks + kApWaves - 1) / kApWaves), (unsigned)kApSlots, (unsigned)cells),
                       dim3(kApThreads), 0, s, a, chunks, thresholds, counts, metric, compute_aos, partial);
  }
  hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)(cells * kApSlots)), dim3(kWave), 0, s, partial, chunks, pr);
  return check_launch("kitti_ap_stats");
}
