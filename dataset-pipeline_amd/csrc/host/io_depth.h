// io_depth.h -- the depth maps GroundTruthCreator writes (write_float_map below) and their reader: width x height raw
// f32, row-major, no header, optionally gzip-compressed with ".gz" appended to the name, one file per image under
// <dir>/<camera folder>/<image name>.  zlib's gz* functions read both: a file without the gzip magic is passed through unchanged.
#pragma once

#include <zlib.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

namespace e3d_host {

// <dir>/<filename(parent(image_file_path))>/<filename(image_file_path)>, the place GroundTruthCreator writes the map of that image
inline std::string depth_map_path(const std::string& dir, const std::string& image_file_path) {
  const size_t s = image_file_path.find_last_of('/');
  const std::string name = s == std::string::npos ? image_file_path : image_file_path.substr(s + 1);
  const std::string parent = s == std::string::npos ? std::string() : image_file_path.substr(0, s);
  const size_t t = parent.find_last_of('/');
  const std::string folder = t == std::string::npos ? parent : parent.substr(t + 1);
  std::string p = dir;
  if (!p.empty() && p.back() != '/') p += '/';
  return p + folder + "/" + name;
}

// Reads the map of one image: depth_map_path, then the same with ".gz".  The payload must be exactly 4 * width * height bytes.
inline bool read_depth_map(const std::string& dir, const std::string& image_file_path, int width, int height, std::vector<float>* out,
                           std::string* err) {
  const std::string raw = depth_map_path(dir, image_file_path), packed = raw + ".gz";
  std::string used = raw;
  gzFile f = gzopen(raw.c_str(), "rb");
  if (!f) { used = packed; f = gzopen(packed.c_str(), "rb"); }
  if (!f) { *err = "Cannot find a depth map: tried " + raw + " and " + packed; return false; }
  gzbuffer(f, 1u << 20);
  const size_t want = sizeof(float) * (size_t)width * (size_t)height;
  out->assign((size_t)width * (size_t)height, 0.f);
  char* dst = reinterpret_cast<char*>(out->data());
  size_t got = 0;
  bool bad = false;
  while (got < want) {                                         // gzread takes an unsigned length
    const unsigned chunk = (unsigned)std::min<size_t>(want - got, 1u << 30);
    const int n = gzread(f, dst + got, chunk);
    if (n < 0) { bad = true; break; }
    if (n == 0) break;
    got += (size_t)n;
  }
  size_t extra = 0;                                            // a longer payload: count it for the message (up to a limit)
  if (!bad && got == want) {
    char tail[4096];
    int n = 0;
    while (extra < (64u << 20) && (n = gzread(f, tail, sizeof tail)) > 0) extra += (size_t)n;
    if (n < 0) bad = true;
  }
  int zerr = Z_OK;
  const std::string zmsg = bad ? std::string(gzerror(f, &zerr)) : std::string();      // (a gzip stream that ends early, for one)
  gzclose(f);
  if (!bad && got == want && extra == 0) return true;
  *err = "Depth map " + used + " holds " + std::to_string(got + extra) + (extra >= (64u << 20) ? "+" : "") + " bytes, expected " +
         std::to_string(want) + " (" + std::to_string(width) + " x " + std::to_string(height) + " f32)" + (bad ? ": " + zmsg : std::string());
  return false;
}

// Writes one map the way read_depth_map finds it: raw f32 under `path`, or gzip-compressed under `path`.gz
inline bool write_float_map(const std::string& path, const std::vector<float>& map, bool compress) {
  if (compress) {
    gzFile f = gzopen((path + ".gz").c_str(), "w8b");
    if (!f) return false;
    const size_t bytes = map.size() * sizeof(float);
    size_t done = 0;
    while (done < bytes) {                                   // gzwrite takes an unsigned length
      const unsigned chunk = (unsigned)std::min<size_t>(bytes - done, 1u << 30);
      if (gzwrite(f, reinterpret_cast<const char*>(map.data()) + done, chunk) != (int)chunk) { gzclose(f); return false; }
      done += chunk;
    }
    return gzclose(f) == Z_OK;
  }
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = fwrite(map.data(), sizeof(float), map.size(), f) == map.size();
  fclose(f);
  return ok;
}

}  // namespace e3d_host
