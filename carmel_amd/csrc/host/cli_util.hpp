// cli_util.hpp — what the two front ends (carmel, forest-em) define identically: the check of a library call's return code,
// print_width, and the file name rule of CARMEL_TRAINED_DIR.
#pragma once
#include <cmath>
#include <cstdlib>
#include <iomanip>
#include <ostream>
#include <stdexcept>
#include <string>
#include "../../../include/carmel_hip.h"
namespace carmel_host {
inline void hip_check(int rc, const char* what) {
  if (rc != CARMEL_HIP_OK) throw std::runtime_error(std::string(what) + ": " + carmel_hip_last_error());
}

// print_width (graehl/shared/print_width.hpp:98-130): a number in at most `width` characters
inline void print_width(std::ostream& os, double d, int width0) {
  if (width0 >= 20 || d == 0. || width0 <= 0) {
    os << d;
    return;
  }
  const std::ios::fmtflags f = os.flags();
  const std::streamsize pr = os.precision();
  int width = width0;
  double pa = d;
  if (d < 0) {
    pa = -d;
    --width;
  }
  auto sig_for_exp = [](int w, int e) {
    const int r = w - (e < 100 ? 2 : 3) - 3;
    return r > 0 ? r : 0;
  };
  const double wholes = std::log10(pa * (1 + 1e-8));
  if (wholes <= width && d == (double)(int)d)
    os << d;
  else if (pa < 1) {
    const int a = (int)-wholes, need = 2 + a;
    if (need >= width)
      os << std::scientific << std::setprecision(sig_for_exp(width, a) - 1) << d;
    else
      os << std::setprecision(width - 2 - a) << d;
  } else {
    const int a = (int)wholes, need = 1 + a;
    if (need > width)
      os << std::scientific << std::setprecision(sig_for_exp(width, a) - 1) << d;
    else
      os << std::fixed << std::setprecision(need + 1 < width ? width - need - 1 : 0) << d;
  }
  os.flags(f);
  os.precision(pr);
}

// <file>.<suffix> (cascade.h:23-32; an empty suffix: the file itself); with CARMEL_TRAINED_DIR set, under that directory by
// the file's base name (tests: write beside nothing read-only)
inline std::string trained_path(const char* file, const std::string& suffix) {
  std::string b = file;
  if (const char* dir = std::getenv("CARMEL_TRAINED_DIR")) {
    size_t sl = b.rfind('/');
    b = std::string(dir) + "/" + (sl == std::string::npos ? b : b.substr(sl + 1));
  }
  return suffix.empty() ? b : b + "." + suffix;
}
}  // namespace carmel_host
