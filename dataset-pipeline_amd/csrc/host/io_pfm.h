// io_pfm.h -- reader of one-channel PFM files ("Pf"), the format of disp0GT.pfm and of the disparity maps stereo methods write:
// "Pf", width, height and scale as text separated by whitespace, one whitespace byte, then height rows of width f32, bottom row
// first.  A negative scale means little-endian samples, a positive one big-endian (swapped here); its magnitude is not applied,
// as Middlebury's readers do not.  The three-channel "PF" is refused with a message.  The result is top row first.
#pragma once

#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

namespace e3d_host {

struct PfmImage {
  int width = 0, height = 0;
  std::vector<float> data;                         // row-major, top row first
  bool empty() const { return data.empty(); }
};

namespace pfm_detail {

// the next whitespace-separated token from `pos`; false at the end of the file
inline bool next_token(const std::vector<uint8_t>& f, size_t* pos, std::string* token) {
  size_t p = *pos;
  while (p < f.size() && isspace(f[p])) ++p;
  token->clear();
  while (p < f.size() && !isspace(f[p])) token->push_back((char)f[p++]);
  *pos = p;
  return !token->empty();
}

// Parses the header: the size, whether the samples are little-endian, and the offset of the first sample.
inline bool parse_header(const std::vector<uint8_t>& f, int* width, int* height, bool* little_endian, size_t* data_begin, std::string* err) {
  size_t pos = 0;
  std::string magic, w, h, scale;
  if (!next_token(f, &pos, &magic) || (magic != "Pf" && magic != "PF")) { *err = "not a PFM file"; return false; }
  if (magic == "PF") { *err = "a three-channel PFM (PF); a one-channel file (Pf) is needed"; return false; }
  if (!next_token(f, &pos, &w) || !next_token(f, &pos, &h) || !next_token(f, &pos, &scale)) { *err = "truncated PFM header"; return false; }
  char* rest = nullptr;
  const long wv = strtol(w.c_str(), &rest, 10);
  const bool w_ok = *rest == 0;
  const long hv = strtol(h.c_str(), &rest, 10);
  const bool h_ok = *rest == 0;
  const double sv = strtod(scale.c_str(), &rest);
  if (!w_ok || !h_ok || *rest != 0 || wv < 1 || hv < 1 || wv > 0x7FFFFFFF || hv > 0x7FFFFFFF || !std::isfinite(sv) || sv == 0.0) { *err = "bad PFM header"; return false; }
  if (pos >= f.size() || !isspace(f[pos])) { *err = "truncated PFM header"; return false; }
  *width = (int)wv; *height = (int)hv; *little_endian = sv < 0.0; *data_begin = pos + 1;
  return true;
}

}  // namespace pfm_detail

// Empty image on failure, the reason in *error.  header_only: the size alone, data stays empty (check width > 0).
inline PfmImage read_pfm(const std::string& path, std::string* error = nullptr, bool header_only = false) {
  PfmImage img;
  std::string err;
  std::ifstream s(path, std::ios::binary);
  if (!s) { if (error) *error = "cannot open " + path; return img; }
  std::vector<uint8_t> f;
  if (header_only) { f.resize(256); s.read(reinterpret_cast<char*>(f.data()), (std::streamsize)f.size()); f.resize((size_t)s.gcount()); }
  else f.assign(std::istreambuf_iterator<char>(s), std::istreambuf_iterator<char>());
  bool little = true;
  size_t begin = 0;
  if (!pfm_detail::parse_header(f, &img.width, &img.height, &little, &begin, &err)) { img = PfmImage(); if (error) *error = path + ": " + err; return img; }
  if (header_only) return img;
  const size_t n = (size_t)img.width * (size_t)img.height;
  if ((f.size() - begin) / 4 < n) { img = PfmImage(); if (error) *error = path + ": truncated PFM data"; return img; }
  img.data.resize(n);
  for (int y = 0; y < img.height; ++y) {
    const uint8_t* row = f.data() + begin + (size_t)(img.height - 1 - y) * img.width * 4;
    float* out = img.data.data() + (size_t)y * img.width;
    if (little) { memcpy(out, row, (size_t)img.width * 4); continue; }
    for (int x = 0; x < img.width; ++x) {
      const uint8_t b[4] = {row[4 * x + 3], row[4 * x + 2], row[4 * x + 1], row[4 * x]};
      memcpy(out + x, b, 4);
    }
  }
  return img;
}

}  // namespace e3d_host
