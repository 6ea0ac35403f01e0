// e3d_read_depth <depth maps dir> <image file path> <width> <height> <out.raw> -- reads the depth map of an image exactly like
// ImageRegistrator --depth_maps_path does (io_depth.h: raw f32 or the same gzip-compressed) and writes it as raw f32.  Used by the
// tests to pin the reader without a GPU; handy for unpacking a compressed map.
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "io_depth.h"

int main(int argc, char** argv) {
  if (argc != 6) { std::cerr << "Usage: " << argv[0] << " <depth maps dir> <image file path> <width> <height> <out.raw>" << std::endl; return 1; }
  const int width = atoi(argv[3]), height = atoi(argv[4]);
  if (width < 1 || height < 1) { std::cerr << "width and height must be positive" << std::endl; return 1; }
  std::vector<float> map;
  std::string err;
  if (!e3d_host::read_depth_map(argv[1], argv[2], width, height, &map, &err)) { std::cerr << err << std::endl; return 1; }
  FILE* f = fopen(argv[5], "wb");
  if (!f) { std::cerr << "cannot write " << argv[5] << std::endl; return 1; }
  const bool ok = fwrite(map.data(), sizeof(float), map.size(), f) == map.size();
  return (fclose(f) == 0 && ok) ? 0 : 1;
}
