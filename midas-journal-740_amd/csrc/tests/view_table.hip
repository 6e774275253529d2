// Host-only test of the source views: resolve_view over every kind x route x projection feature and every pair of kinds,
// framed_desc of every kind against cuberille_region_desc and the padded description.  No device is touched: the program
// includes the host layer and never creates a context through the ABI.  Built plain for the suite (tests/test_view_table.py);
// the same source under -Xarch_host -fsanitize=address,undefined is the sanitizer run of this code.
#include "../cuberille_api.hip"

#include <cstdio>

namespace {

int failures = 0;
#define EXPECT(cond, ...)                                                    \
  do {                                                                       \
    if (!(cond)) {                                                           \
      failures++;                                                            \
      std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond);        \
      std::printf(__VA_ARGS__);                                              \
      std::printf("\n");                                                     \
    }                                                                        \
  } while (0)

const char *const kWord[4] = {"", "border", "region", "band"};
const char *const kFn[4] = {"", "cuberille_set_border", "cuberille_set_region", "cuberille_set_band"};

cuberille_image_desc image(int64_t nx, int64_t ny, int64_t nz, int64_t s0 = 0, int64_t s1 = 0, int64_t s2 = 0) {
  cuberille_image_desc d{};
  d.pixel_type = CUBERILLE_PIX_F32;
  d.dims[0] = nx; d.dims[1] = ny; d.dims[2] = nz;
  d.index_start[0] = s0; d.index_start[1] = s1; d.index_start[2] = s2;
  for (int i = 0; i < 3; i++) { d.spacing[i] = 1.0 + i; d.origin[i] = -3.0 * i; d.direction[i * 4] = 1.0; }
  return d;
}

void set(cuberille_ctx &c, int kind) {
  if (kind == VIEW_BORDER) { c.padWidth = 1; c.padValue = 0.0; }
  if (kind == VIEW_REGION) { c.regionOn = true; for (int i = 0; i < 3; i++) { c.regionStart[i] = 1; c.regionSize[i] = 2; } }
  if (kind == VIEW_BAND) { c.bandOn = true; c.bandV[0] = 1; c.bandV[1] = 2; c.bandV[2] = 1; c.bandVi[0] = 1; c.bandVi[1] = 2; c.bandVi[2] = 1; }
}

// the message names exactly the settings in `kinds` (bit k), each by word and by function
void names_only(const char *why, unsigned kinds, const char *what) {
  for (int k = VIEW_BORDER; k <= VIEW_BAND; k++) {
    const bool word = std::strstr(why, kWord[k]) != nullptr, fn = std::strstr(why, kFn[k]) != nullptr;
    if (kinds & (1u << k)) EXPECT(word && fn, "%s: \"%s\" should name the %s", what, why, kWord[k]);
    else EXPECT(!word && !fn, "%s: \"%s\" should not name the %s", what, why, kWord[k]);
  }
}

bool same(const cuberille_image_desc &a, const cuberille_image_desc &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

void routes_and_features() {
  const cuberille_image_desc img = image(5, 4, 3);
  // what each route offers of each kind (ROUTE_WARM_UP reserves: the band changes no size and is not looked at)
  const bool offered[4][N_ROUTES] = {{true, true, true, true, true, true, true},
                                     {true, true, false, false, true, false, true},
                                     {true, true, false, false, false, false, true},
                                     {true, true, false, false, false, false, true}};
  for (int kind = VIEW_WHOLE; kind <= VIEW_BAND; kind++)
    for (int route = 0; route < N_ROUTES; route++)
      for (int feature = 0; feature < 6; feature++) {      // 0 none, 1 projection off, 2 B-spline, 3 held gradient, 4 recursive Gaussian, 5 the two branches
        for (int variant = 1; variant <= (feature == 5 ? 2 : 1); variant++) {
          cuberille_ctx c;
          set(c, kind);
          Params p{};
          p.project = feature != 1;
          if (feature == 2) c.interp = CUBERILLE_INTERP_BSPLINE;
          if (feature == 3) c.holdGradient = true;
          if (feature == 4) p.gradVariant = CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN;
          if (feature == 5) p.variant = variant;
          View v{};
          v.kind = -1;
          const char *why = nullptr;
          const int rc = resolve_view(&c, &img, p, (Route)route, &v, &why);
          char what[96];
          std::snprintf(what, sizeof what, "kind %d route %d feature %d", kind, route, feature);
          const bool featured = feature >= 2 && kind != VIEW_WHOLE && route != ROUTE_WARM_UP;
          if (offered[kind][route] && !featured) {
            const int expect = kind == VIEW_BAND && route == ROUTE_WARM_UP ? (int)VIEW_WHOLE : kind;
            EXPECT(rc == CUBERILLE_OK && v.kind == expect, "%s: rc %d kind %d \"%s\"", what, rc, v.kind, why);
          } else {
            EXPECT(rc == CUBERILLE_ERR_ARGUMENT, "%s: rc %d", what, rc);
            names_only(why, 1u << kind, what);
          }
        }
      }
}

void pairs() {
  const cuberille_image_desc img = image(5, 4, 3);
  for (int a = VIEW_BORDER; a <= VIEW_BAND; a++)
    for (int b = a + 1; b <= VIEW_BAND; b++)
      for (int route : {ROUTE_DEVICE, ROUTE_HOST, ROUTE_STREAM}) {
        cuberille_ctx c;
        set(c, a);
        set(c, b);
        View v{};
        const char *why = nullptr;
        const int rc = resolve_view(&c, &img, Params{}, (Route)route, &v, &why);
        EXPECT(rc == CUBERILLE_ERR_ARGUMENT, "pair %d %d: rc %d", a, b, rc);
        // (a stream takes neither a region nor a band: its refusal of the one it meets first, the region, comes before the pair's)
        const unsigned named = route != ROUTE_STREAM ? (1u << a) | (1u << b) : 1u << (a == VIEW_REGION || b == VIEW_REGION ? VIEW_REGION : VIEW_BAND);
        names_only(why, named, "pair");
      }
  // all three: the region with the border, and no word of the band
  cuberille_ctx c;
  for (int k = VIEW_BORDER; k <= VIEW_BAND; k++) set(c, k);
  View v{};
  const char *why = nullptr;
  EXPECT(resolve_view(&c, &img, Params{}, ROUTE_HOST, &v, &why) == CUBERILLE_ERR_ARGUMENT, "all three");
  names_only(why, (1u << VIEW_BORDER) | (1u << VIEW_REGION), "all three");
}

void validators() {
  const char *why = "";
  View v{};
  // the border's value against an integer pixel type; the limits of the image with its ring
  cuberille_ctx c;
  set(c, VIEW_BORDER);
  c.padValue = 256.0;
  cuberille_image_desc u8 = image(5, 4, 3);
  u8.pixel_type = CUBERILLE_PIX_U8;
  EXPECT(resolve_view(&c, &u8, Params{}, ROUTE_DEVICE, &v, &why) == CUBERILLE_ERR_ARGUMENT, "ring value 256 in uint8");
  names_only(why, 1u << VIEW_BORDER, "ring value");
  c.padValue = 255.0;
  EXPECT(resolve_view(&c, &u8, Params{}, ROUTE_DEVICE, &v, &why) == CUBERILLE_OK, "ring value 255 in uint8: %s", why);
  cuberille_image_desc low = image(5, 4, 3, -(1LL << 30), 0, 0);
  EXPECT(resolve_view(&c, &low, Params{}, ROUTE_DEVICE, &v, &why) == CUBERILLE_ERR_LIMIT, "a ring below -2^30");
  cuberille_image_desc wide = image(0x7fffffffLL - 1, 4, 3);
  EXPECT(resolve_view(&c, &wide, Params{}, ROUTE_WARM_UP, &v, &why) == CUBERILLE_ERR_LIMIT, "a ring past 2^31-1");
  // the band's values against the pixel type, by band_check
  cuberille_ctx b;
  set(b, VIEW_BAND);
  b.bandV[1] = 256.0; b.bandVi[1] = 256;
  EXPECT(resolve_view(&b, &u8, Params{}, ROUTE_HOST, &v, &why) == CUBERILLE_ERR_ARGUMENT, "band bound 256 in uint8");
  names_only(why, 1u << VIEW_BAND, "band bound");
  b.bandV[0] = 3.0; b.bandV[1] = 2.0; b.bandVi[0] = 3; b.bandVi[1] = 2;
  EXPECT(resolve_view(&b, &u8, Params{}, ROUTE_HOST, &v, &why) == CUBERILLE_ERR_ARGUMENT, "band lower above upper");
  const cuberille_image_desc f32 = image(5, 4, 3);
  EXPECT(resolve_view(&b, &f32, Params{}, ROUTE_WARM_UP, &v, &why) == CUBERILLE_OK && v.kind == VIEW_WHOLE, "a warm-up does not read the band");
  // the region against the buffer, by region_check
  cuberille_ctx r;
  set(r, VIEW_REGION);
  r.regionSize[0] = 5;
  EXPECT(resolve_view(&r, &f32, Params{}, ROUTE_DEVICE, &v, &why) == CUBERILLE_ERR_ARGUMENT, "a box that leaves the buffer");
  names_only(why, 1u << VIEW_REGION, "box leaves the buffer");
}

void frames() {
  const int64_t dimsOf[2][3] = {{5, 4, 3}, {70, 3, 2}};
  for (const auto &n : dimsOf) {
    const cuberille_image_desc img = image(n[0], n[1], n[2], 7, -2, 100);
    // whole and band: the image itself
    View v{};
    EXPECT(same(framed_desc(v, &img), img), "whole");
    v.kind = VIEW_BAND;
    EXPECT(same(framed_desc(v, &img), img), "band");
    // border: the region grown by one on every side, everything else the image's
    v.kind = VIEW_BORDER;
    cuberille_image_desc padded = img;
    for (int i = 0; i < 3; i++) { padded.dims[i] += 2; padded.index_start[i] -= 1; }
    EXPECT(same(framed_desc(v, &img), padded), "border");
    // region: cuberille_region_desc's, for the whole buffer, an inner box and a box touching each face
    for (int face = -1; face < 7; face++) {
      int64_t start[3], size[3];
      for (int i = 0; i < 3; i++) {
        const bool thin = n[i] < 3;                       // (an axis of 2: the box is its first or its last voxel)
        start[i] = thin ? 0 : 1; size[i] = thin ? 1 : n[i] - 2;
        if (face == 2 * i) start[i] = 0;                  // touches the low face
        if (face == 2 * i + 1) start[i] = n[i] - size[i]; // touches the high face
        if (face == 6) { start[i] = 0; size[i] = n[i]; }  // the buffer itself
      }
      cuberille_ctx c;
      c.regionOn = true;
      for (int i = 0; i < 3; i++) { c.regionStart[i] = start[i]; c.regionSize[i] = size[i]; }
      const char *why = "";
      EXPECT(resolve_view(&c, &img, Params{}, ROUTE_DEVICE, &v, &why) == CUBERILLE_OK && v.kind == VIEW_REGION, "face %d: %s", face, why);
      cuberille_image_desc want;
      EXPECT(cuberille_region_desc(&img, start, size, &want) == CUBERILLE_OK, "face %d", face);
      EXPECT(same(framed_desc(v, &img), want), "region, face %d", face);
      EXPECT(v.rowPitch == n[0] && v.slicePitch == n[0] * n[1], "the buffer's pitches, face %d", face);
      EXPECT((v.pitched != 0) == (size[0] != n[0] || size[1] != n[1]), "pitched, face %d", face);
      // ... and what cuberille_extract_host hands on behind its upload of the box: the box, contiguous, at its own index
      const View applied = applied_region(want);
      EXPECT(same(framed_desc(applied, &want), want) && !applied.pitched && applied.rowPitch == size[0] &&
             applied.slicePitch == size[0] * size[1] && applied.start[0] == 0 && applied.start[1] == 0 && applied.start[2] == 0,
             "applied region, face %d", face);
    }
  }
  // a start index at the limit of +-2^30 and one beyond it, for the box and for the ring
  for (int sign = -1; sign <= 1; sign += 2)
    for (int beyond = 0; beyond < 2; beyond++) {
      const int64_t at = sign * (1LL << 30);
      // the buffer starts `1` inside the limit and the box at position 1 (2 when beyond): the box's index is the limit (or past it)
      const cuberille_image_desc img = image(5, 4, 3, sign > 0 ? at - 1 : at, 0, 0);
      cuberille_ctx c;
      c.regionOn = true;
      for (int i = 0; i < 3; i++) { c.regionStart[i] = 0; c.regionSize[i] = 2; }
      c.regionStart[0] = sign > 0 ? 1 + beyond : 0;
      cuberille_image_desc low = img;
      if (sign < 0 && beyond) low.index_start[0] = at - 1;
      View v{};
      const char *why = "";
      const int rc = resolve_view(&c, &low, Params{}, ROUTE_DEVICE, &v, &why);
      cuberille_image_desc want;
      const int rd = cuberille_region_desc(&low, c.regionStart, c.regionSize, &want);
      EXPECT(rc == rd && rc == (beyond ? CUBERILLE_ERR_LIMIT : CUBERILLE_OK), "region at %+d * 2^30, beyond %d: rc %d, %d \"%s\"", sign, beyond, rc, rd, why);
      if (!rc) EXPECT(same(framed_desc(v, &low), want) && want.index_start[0] == at, "region at the limit");
      if (sign < 0) {
        // the ring reaches one index below the buffer's: -2^30 + 1 is the lowest start that takes a border
        cuberille_ctx b;
        set(b, VIEW_BORDER);
        const cuberille_image_desc ring = image(5, 4, 3, at + (beyond ? 0 : 1), 0, 0);
        const int rb = resolve_view(&b, &ring, Params{}, ROUTE_DEVICE, &v, &why);
        EXPECT(rb == (beyond ? CUBERILLE_ERR_LIMIT : CUBERILLE_OK), "border at -2^30, beyond %d: rc %d", beyond, rb);
        if (!rb) EXPECT(framed_desc(v, &ring).index_start[0] == at, "the ring's index at the limit");
      }
    }
}

}  // namespace

int main() {
  routes_and_features();
  pairs();
  validators();
  frames();
  std::printf(failures ? "view_table: %d check(s) FAILED\n" : "view_table ok\n", failures);
  return failures ? 1 : 0;
}
