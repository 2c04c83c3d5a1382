// workspace_check.cpp -- stand-alone check of csrc/workspace.h on the host (built with ASan + UBSan by tests/test_workspace_host.py).
// Three layouts in the shapes the library's call sites have -- mixed element types with a fixed block taken last, a region shared by
// two users through a max, an array of pieces with empty ones between -- are measured, then carved into a heap buffer of EXACTLY the
// measured size: every piece must lie inside the buffer, start on a 256-byte granule from the base and end before the next begins,
// the carve must end at the measured size, and every byte of every piece is written (a piece past the end is ASan's to report).
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "workspace.h"

namespace ngpde {
static char last_error[256];
int32_t fail(int32_t code, const char *fmt, ...) {   // (the header only declares it: the library's records the message for ngpde_last_error)
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(last_error, sizeof(last_error), fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace ngpde

using namespace ngpde;

namespace {

int failures = 0;
void check(bool ok, const char *what) {
  if (ok) return;
  ++failures;
  std::fprintf(stderr, "FAILED %s\n", what);
}

struct Piece {
  char *at;
  size_t bytes;
};
struct Recorder {   // takes through the Workspace and notes each piece
  Workspace &w;
  std::vector<Piece> pieces;
  template <class T>
  T *take(size_t count) {
    T *p = w.take<T>(count);
    pieces.push_back({reinterpret_cast<char *>(p), count * sizeof(T)});
    return p;
  }
};

// (a) the traversals' shape: 64-bit words, floats, a fixed 256-byte block last
void layout_a(Recorder &r, size_t n) {
  r.take<unsigned long long>(n);
  r.take<unsigned long long>(n);
  r.take<float>(3 * n + 1);
  r.take<int32_t>(64);
}
// (b) the GCN pullback's: two equal buffers and a third region that serves the larger of two users
void layout_b(Recorder &r, size_t n) {
  r.take<float>(n * 7);
  r.take<float>(n * 7);
  r.take<float>(std::max<size_t>(5 * n, 129));
  r.take<char>(256);
  r.take<float>(n);
}
// (c) the deep edge-MLP's: an array of pieces, some of them empty, odd byte counts
void layout_c(Recorder &r, size_t n) {
  for (size_t l = 0; l < 5; ++l) r.take<char>(l % 2 ? 0 : n * (l + 1) + 1);
  r.take<double>(n);
}

template <class Layout>
void run(const char *name, Layout layout, size_t n) {
  Workspace measure;
  Recorder m{measure, {}};
  layout(m, n);
  const size_t need = measure.bytes();
  check(need % kGranule == 0, "the measured size is a whole number of granules");
  for (const Piece &p : m.pieces) check(p.at == nullptr, "a measuring pass returns nullptr");

  char *base = static_cast<char *>(std::aligned_alloc(kGranule, std::max(need, kGranule)));
  // (aligned_alloc wants a size that is a multiple of the alignment: need is one; an empty layout gets one granule it never touches)
  Workspace carve(base);
  Recorder c{carve, {}};
  layout(c, n);
  check(carve.bytes() == need, "the carve ends at the measured size");
  check(c.pieces.size() == m.pieces.size(), "both passes take the same pieces");
  char *end_of_last = base;
  for (const Piece &p : c.pieces) {
    const size_t off = (size_t)(p.at - base);
    check(p.at >= base && off + p.bytes <= need, "a piece lies inside the buffer");
    check(off % kGranule == 0, "a piece starts on a granule");
    check(p.at >= end_of_last, "a piece begins where the one before has ended");
    std::memset(p.at, 0x5a, p.bytes);
    end_of_last = p.at + p.bytes;
  }
  if (failures) std::fprintf(stderr, "  (layout %s, n = %zu, %zu bytes)\n", name, n, need);
  std::free(base);
}

}  // namespace

int main() {
  for (size_t n : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)4097}) {
    run("a", layout_a, n);
    run("b", layout_b, n);
    run("c", layout_c, n);
  }
  check(round_up256(0) == 0 && round_up256(1) == 256 && round_up256(256) == 256 && round_up256(257) == 512, "round_up256");

  // check_workspace: too small and NULL raise NGPDE_ERR_WORKSPACE with the one wording, a misaligned base NGPDE_ERR_INVALID_ARGUMENT
  alignas(256) static char buf[512];
  check(check_workspace("f", buf, 512, 512, 16) == NGPDE_OK, "an exact fit passes");
  check(check_workspace("f", buf, 511, 512, 1) == NGPDE_ERR_WORKSPACE && std::strstr(last_error, "f: workspace of 511 bytes, 512 needed"),
        "a short workspace is refused with the sizes");
  check(check_workspace("f", nullptr, 512, 0, 1) == NGPDE_ERR_WORKSPACE, "a NULL workspace is refused");
  check(check_workspace("f", buf + 8, 256, 256, 16) == NGPDE_ERR_INVALID_ARGUMENT && std::strstr(last_error, "16-byte aligned"),
        "a misaligned base is refused");
  check(check_workspace("f", buf + 8, 256, 256, 8) == NGPDE_OK && check_workspace("f", buf + 1, 256, 256, 1) == NGPDE_OK,
        "align 1 tests nothing, align 8 passes a multiple of 8");

  if (failures) {
    std::fprintf(stderr, "%d failed checks\n", failures);
    return 1;
  }
  std::printf("workspace_check ok\n");
  return 0;
}
