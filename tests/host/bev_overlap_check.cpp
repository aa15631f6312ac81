// Host check of csrc/bev_overlap.h (the text K20's kernels compile), meant to be built with -fsanitize=address,undefined
// and -ffp-contract=off (the library's own setting) and run by tests/test_nms_degenerate_cpu.py.
//
//   bev_overlap_check [identical_pairs [pairs_per_family]]        (defaults 2 000 000 and 50 000)
//
// It feeds the fp32 routine the degenerate pair families of tests/test_nms_degenerate_gpu.py plus `identical_pairs` boxes
// tested against themselves, both argument orders, and compares every fp32 IoU with a float64 value computed here: the
// closed form where the family has one, else a float64 Sutherland-Hodgman clip of the same (fp32-rounded) boxes.  The
// float64 clip is itself compared with the closed forms.  Bound per pair (docs/kernels/K17_K20_K24_refine_tail.md):
//   tol = 64 * 2^-23 * max|coordinate| / min side
// the 0.05 m-in-3 x 12 m family uses the bound of its own geometry instead.  Non-finite and non-positive boxes must give
// an IoU that is not > 0.  Prints the worst vertex count of the clip polygon and how many pairs went beyond eight; exits
// 1 on any violation or when the count exceeds BEV_CLIP_CAP or the header's BEV_CLIP_WORST_SEEN.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "../../fullysparsefusion_amd/csrc/bev_overlap.h"

namespace {

constexpr double PI = 3.14159265358979323846;
constexpr double EPS32 = 1.0 / 8388608.0;  // 2^-23

struct Box {
  double cx, cy, w, l, yaw;
};

void to_f32(const Box& b, float* o) {
  o[0] = (float)(b.cx - b.w / 2);
  o[1] = (float)(b.cy - b.l / 2);
  o[2] = (float)(b.cx + b.w / 2);
  o[3] = (float)(b.cy + b.l / 2);
  o[4] = (float)b.yaw;
}

// centre of `b` moved by (ox, oy) in b's own frame: the kernel's corner = centre + [[c, s], [-s, c]] * offset
void shift_local(Box& b, const Box& frame, double ox, double oy) {
  const double c = std::cos(frame.yaw), s = std::sin(frame.yaw);
  b.cx = frame.cx + c * ox + s * oy;
  b.cy = frame.cy - s * ox + c * oy;
}

// float64 overlap of two fp32 boxes: A's corners into B's frame, clipped against B's four sides (64 slots)
double overlap64(const float* a, const float* b) {
  const double bcx = 0.5 * ((double)b[0] + b[2]), bcy = 0.5 * ((double)b[1] + b[3]);
  const double bhx = 0.5 * ((double)b[2] - b[0]), bhy = 0.5 * ((double)b[3] - b[1]);
  const double acx = 0.5 * ((double)a[0] + a[2]), acy = 0.5 * ((double)a[1] + a[3]);
  const double ahx = 0.5 * ((double)a[2] - a[0]), ahy = 0.5 * ((double)a[3] - a[1]);
  if (!(bhx > 0) || !(bhy > 0) || !(ahx > 0) || !(ahy > 0)) return 0.0;
  const double ca = std::cos((double)a[4]), sa = std::sin((double)a[4]), cb = std::cos((double)b[4]), sb = std::sin((double)b[4]);
  double px[64], py[64], qx[64], qy[64];
  const double ox[4] = {-ahx, ahx, ahx, -ahx}, oy[4] = {-ahy, -ahy, ahy, ahy};
  for (int k = 0; k < 4; ++k) {
    const double wx = acx + ca * ox[k] + sa * oy[k] - bcx, wy = acy - sa * ox[k] + ca * oy[k] - bcy;
    px[k] = cb * wx - sb * wy;
    py[k] = sb * wx + cb * wy;
  }
  int n = 4;
  for (int side = 0; side < 4; ++side) {
    const double lim = side < 2 ? bhx : bhy, sgn = (side & 1) ? -1.0 : 1.0;
    int m = 0;
    for (int k = 0; k < n; ++k) {
      const int k2 = (k + 1) % n;
      const double c0 = sgn * (side < 2 ? px[k] : py[k]), c1 = sgn * (side < 2 ? px[k2] : py[k2]);
      const bool in0 = c0 <= lim, in1 = c1 <= lim;
      if (in0 && m < 64) { qx[m] = px[k]; qy[m] = py[k]; ++m; }
      if (in0 != in1 && m < 64) {
        const double t = (lim - c0) / (c1 - c0);
        qx[m] = px[k] + t * (px[k2] - px[k]);
        qy[m] = py[k] + t * (py[k2] - py[k]);
        ++m;
      }
    }
    n = m;
    for (int k = 0; k < n; ++k) { px[k] = qx[k]; py[k] = qy[k]; }
    if (n < 3) return 0.0;
  }
  double area = 0;
  for (int k = 1; k + 1 < n; ++k) area += (px[k] - px[0]) * (py[k + 1] - py[0]) - (px[k + 1] - px[0]) * (py[k] - py[0]);
  return 0.5 * std::fabs(area);
}

double area64(const float* b) { return ((double)b[2] - b[0]) * ((double)b[3] - b[1]); }

double iou_from_overlap(const float* a, const float* b, double ov) {
  return ov / std::fmax(area64(a) + area64(b) - ov, 1e-8);
}

double pair_tol(const float* a, const float* b) {
  double m = 0, side = 1e300;
  for (const float* q : {a, b}) {
    for (int k = 0; k < 4; ++k) m = std::fmax(m, std::fabs((double)q[k]));
    side = std::fmin(side, std::fmin((double)q[2] - q[0], (double)q[3] - q[1]));
  }
  return 64.0 * EPS32 * m / side;
}

enum Family {
  IDENTICAL, PI_FLIP, SWAP_WL, JITTER, NESTED_SAME_YAW, NESTED_OTHER_YAW, SLID, SHARED_EDGE, SHARED_CORNER, CROSS90, EXACT_YAW,
  TINY_IN_HUGE, GENERIC, NUM_FAMILIES
};
const char* const NAMES[NUM_FAMILIES] = {"identical", "pi_flip", "swap_wl", "jitter", "nested_same_yaw", "nested_other_yaw", "slid",
                                         "shared_edge", "shared_corner", "cross90", "exact_yaw", "tiny_in_huge", "generic"};

struct Rng {
  std::mt19937_64 g;
  explicit Rng(uint64_t s) : g(s) {}
  double u(double lo, double hi) { return lo + (hi - lo) * std::generate_canonical<double, 53>(g); }
  int pick(int n) { return (int)(g() % (uint64_t)n); }
};

// one pair of `fam`; returns the closed-form IoU of the ideal pair, NaN when the family has none
double make_pair(Family fam, Rng& r, float* fa, float* fb) {
  Box a{r.u(-90, 90), r.u(-90, 90), r.u(0.5, 3.0), r.u(0.5, 12.0), r.u(-3.2, 3.2)};
  Box b = a;
  double iou = std::numeric_limits<double>::quiet_NaN();
  switch (fam) {
    case IDENTICAL: iou = 1; break;
    case PI_FLIP: b.yaw = a.yaw + PI; iou = 1; break;
    case SWAP_WL: b.w = a.l; b.l = a.w; b.yaw = a.yaw + PI / 2; iou = 1; break;
    case JITTER: {
      const double j = std::pow(10.0, r.u(-6, -4));
      b.cx += r.u(-j, j); b.cy += r.u(-j, j); b.w += r.u(-j, j); b.l += r.u(-j, j); b.yaw += r.u(-j, j);
      break;
    }
    case NESTED_SAME_YAW: {
      a.w = r.u(1.0, 3.0); a.l = r.u(1.0, 12.0);
      const double s = r.u(0.5, 0.9);
      b.w = a.w * s; b.l = a.l * s;
      shift_local(b, a, r.u(-0.9, 0.9) * (a.w - b.w) / 2, r.u(-0.9, 0.9) * (a.l - b.l) / 2);
      iou = b.w * b.l / (a.w * a.l);
      break;
    }
    case NESTED_OTHER_YAW: {
      a.w = r.u(2.0, 3.0); a.l = r.u(2.0, 12.0);
      b.w = r.u(0.5, 0.9); b.l = r.u(0.5, 0.9); b.yaw = r.u(-3.2, 3.2);  // half diagonal <= 0.64 < 0.9 (a.w / 2 - 0.1)
      shift_local(b, a, r.u(-1, 1) * (a.w / 2 - 0.7), r.u(-1, 1) * (a.l / 2 - 0.7));
      iou = b.w * b.l / (a.w * a.l);
      break;
    }
    case SLID: {
      const double d = r.u(0, 1.2) * a.l;
      shift_local(b, a, 0, d);
      const double ov = a.w * std::fmax(a.l - d, 0.0);
      iou = ov / (2 * a.w * a.l - ov);
      break;
    }
    case SHARED_EDGE: shift_local(b, a, 0, a.l); iou = 0; break;
    case SHARED_CORNER: shift_local(b, a, a.w, a.l); iou = 0; break;
    case CROSS90: {
      b.yaw = a.yaw + PI / 2;
      const double s = std::fmin(a.w, a.l), ov = s * s;
      iou = ov / (2 * a.w * a.l - ov);
      break;
    }
    case EXACT_YAW: {
      const double yaws[4] = {0, PI / 2, -PI / 2, PI};
      const int ia = r.pick(4), ib = r.pick(4);
      a.yaw = yaws[ia]; b.yaw = yaws[ib];
      b.w = r.u(0.5, 3.0); b.l = r.u(0.5, 12.0);
      b.cx = a.cx + r.u(-2, 2); b.cy = a.cy + r.u(-6, 6);
      const bool ta = ia == 1 || ia == 2, tb = ib == 1 || ib == 2;  // a quarter turn swaps the extents
      const double aw = ta ? a.l : a.w, al = ta ? a.w : a.l, bw = tb ? b.l : b.w, bl = tb ? b.w : b.l;
      const double ox = std::fmax(std::fmin(a.cx + aw / 2, b.cx + bw / 2) - std::fmax(a.cx - aw / 2, b.cx - bw / 2), 0.0);
      const double oy = std::fmax(std::fmin(a.cy + al / 2, b.cy + bl / 2) - std::fmax(a.cy - al / 2, b.cy - bl / 2), 0.0);
      iou = ox * oy / (a.w * a.l + b.w * b.l - ox * oy);
      break;
    }
    case TINY_IN_HUGE: {
      a.w = 3; a.l = 12;
      b.w = 0.05; b.l = 0.05; b.yaw = r.u(-3.2, 3.2);
      shift_local(b, a, r.u(-1.4, 1.4), r.u(-5.9, 5.9));
      iou = b.w * b.l / (a.w * a.l);
      break;
    }
    case GENERIC: {
      b.w = r.u(0.5, 3.0); b.l = r.u(0.5, 12.0); b.yaw = r.u(-3.2, 3.2);
      b.cx = a.cx + r.u(-3, 3); b.cy = a.cy + r.u(-3, 3);
      break;
    }
    default: break;
  }
  to_f32(a, fa);
  to_f32(b, fb);
  return iou;
}

struct Stats {
  long pairs = 0, over8 = 0, bad = 0;
  int worst = 0;
  double worst_ratio = 0;
};

// both argument orders of one pair against `want` within `tol`
void check_pair(const float* a, const float* b, double want, double tol, Stats& s, const char* what) {
  for (int order = 0; order < 2; ++order) {
    const float* p = order ? b : a;
    const float* q = order ? a : b;
    int nv = 0;
    const double got = fsf::iou_bev(p, q, 1, &nv);
    if (nv > s.worst) s.worst = nv;
    if (nv > 8) ++s.over8;
    const double err = std::fabs(got - want);
    if (err / tol > s.worst_ratio) s.worst_ratio = err / tol;
    if (!(err <= tol)) {
      if (s.bad++ < 10)
        std::printf("MISMATCH %s order %d: fp32 %.9g float64 %.17g tol %.3g  a=(%.9g %.9g %.9g %.9g %.9g) b=(%.9g %.9g %.9g %.9g %.9g)\n",
                    what, order, got, want, tol, p[0], p[1], p[2], p[3], p[4], q[0], q[1], q[2], q[3], q[4]);
    }
    ++s.pairs;
  }
}

}  // namespace

int main(int argc, char** argv) {
  const long n_identical = argc > 1 ? std::atol(argv[1]) : 2000000;
  const long n_family = argc > 2 ? std::atol(argv[2]) : 50000;
  long bad = 0;
  int worst = 0;
  long over8 = 0, pairs = 0;
  for (int f = 0; f < NUM_FAMILIES; ++f) {
    Rng r(1000 + f);
    Stats s;
    long bad_ref = 0;
    for (long i = 0; i < n_family; ++i) {
      float a[5], b[5];
      const double closed = make_pair((Family)f, r, a, b);
      const double clip = iou_from_overlap(a, b, overlap64(a, b));
      double tol = pair_tol(a, b);
      if (f == TINY_IN_HUGE) {
        // overlap error <= perimeter of the small box x vertex error (16 ulp of the largest coordinate), over the union >= the big area
        double m = 0;
        for (int k = 0; k < 4; ++k) m = std::fmax(m, std::fmax(std::fabs((double)a[k]), std::fabs((double)b[k])));
        tol = 4 * 0.05 * 16.0 * EPS32 * m / 36.0;
      }
      if (!std::isnan(closed) && !(std::fabs(clip - closed) <= tol)) {  // the float64 clip against the closed form
        if (bad_ref++ < 10) std::printf("REFERENCE %s: float64 clip %.17g closed form %.17g tol %.3g\n", NAMES[f], clip, closed, tol);
      }
      check_pair(a, b, std::isnan(closed) ? clip : closed, tol, s, NAMES[f]);
    }
    std::printf("%-17s pairs %8ld  worst vertices %2d  beyond eight %6ld  worst |err| / tol %.3f  mismatches %ld  reference mismatches %ld\n",
                NAMES[f], s.pairs, s.worst, s.over8, s.worst_ratio, s.bad, bad_ref);
    bad += s.bad + bad_ref;
    if (s.worst > worst) worst = s.worst;
    over8 += s.over8;
    pairs += s.pairs;
  }
  {  // the issue's population: centres within +-50 m, sides 0.3-3 m by 0.3-12 m, yaw uniform in +-3.2, each box against itself
    Rng r(7);
    Stats s;
    for (long i = 0; i < n_identical; ++i) {
      const Box a{r.u(-50, 50), r.u(-50, 50), r.u(0.3, 3.0), r.u(0.3, 12.0), r.u(-3.2, 3.2)};
      float fa[5];
      to_f32(a, fa);
      int nv = 0;
      const double got = fsf::iou_bev(fa, fa, 1, &nv);
      const double tol = pair_tol(fa, fa), err = std::fabs(got - 1.0);
      if (nv > s.worst) s.worst = nv;
      if (nv > 8) ++s.over8;
      if (err / tol > s.worst_ratio) s.worst_ratio = err / tol;
      if (!(err <= tol) && s.bad++ < 10)
        std::printf("MISMATCH identical: fp32 %.9g tol %.3g  a=(%.9g %.9g %.9g %.9g %.9g)\n", got, tol, fa[0], fa[1], fa[2], fa[3], fa[4]);
      ++s.pairs;
    }
    std::printf("%-17s pairs %8ld  worst vertices %2d  beyond eight %6ld  worst |err| / tol %.3f  mismatches %ld\n", "identical_2m", s.pairs,
                s.worst, s.over8, s.worst_ratio, s.bad);
    bad += s.bad;
    if (s.worst > worst) worst = s.worst;
    over8 += s.over8;
    pairs += s.pairs;
  }
  {  // the box the issue names, against itself
    const float a[5] = {-24.6383247f, 5.27780294f, -21.7259178f, 10.7708778f, 1.31265569f};
    int nv = 0;
    const double got = fsf::iou_bev(a, a, 1, &nv);
    std::printf("named box: %d vertices, IoU %.9g\n", nv, got);
    if (!(std::fabs(got - 1.0) <= pair_tol(a, a))) ++bad;
    if (nv > worst) worst = nv;
  }
  {  // non-finite / non-positive boxes: neither suppress nor are suppressed, i.e. the IoU is never > 0, in either order
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float good[5] = {0.f, 0.f, 2.f, 4.f, 0.3f};
    const float odd[][5] = {{0, 0, 2, 4, nan},  {nan, 0, 2, 4, 0.3f}, {0, 0, nan, 4, 0.3f}, {0, 0, inf, 4, 0.3f},  {-inf, 0, 2, 4, 0.3f},
                            {0, -inf, 2, inf, 0.3f}, {0, 0, 2, 4, inf},  {1, 0, 1, 4, 0.3f},   {2, 0, 0, 4, 0.3f},    {0, 0, 2, 4, 1e30f},
                            {-inf, -inf, inf, inf, 0.f}, {nan, nan, nan, nan, nan}};
    for (const auto& o : odd) {  // (the rotated path: what K20's contract covers)
      int nv = 0;
      const float v[3] = {fsf::iou_bev(o, good, 1, &nv), fsf::iou_bev(good, o, 1, &nv), fsf::iou_bev(o, o, 1, &nv)};
      if (nv > worst) worst = nv;
      const bool huge_yaw = o[4] == 1e30f;  // a finite yaw of any size is an ordinary box
      for (int k = 0; k < 3; ++k) {
        if (huge_yaw ? !(v[k] >= 0.f && v[k] <= 1.0001f) : (v[k] > 0.f)) {
          std::printf("ODD BOX (%g %g %g %g %g) case %d: IoU %g\n", o[0], o[1], o[2], o[3], o[4], k, v[k]);
          ++bad;
        }
      }
    }
  }
  std::printf("worst_vertices=%d beyond_eight=%ld pairs=%ld capacity=%d worst_seen=%d mismatches=%ld\n", worst, over8, pairs,
              fsf::BEV_CLIP_CAP, fsf::BEV_CLIP_WORST_SEEN, bad);
  return (bad == 0 && worst <= fsf::BEV_CLIP_CAP && worst <= fsf::BEV_CLIP_WORST_SEEN) ? 0 : 1;
}
