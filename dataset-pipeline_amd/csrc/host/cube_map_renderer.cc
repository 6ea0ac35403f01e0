// CubeMapRenderer -- drop-in replacement of the reference tool (src/exe/cube_map_renderer.cc:113-399): renders the six cube map
// faces (front, left, back, right, down, up) of a coloured laser scan, given in the scanner's frame, as colour images and depth
// maps for the SfM step.  The z-buffer, the fill-in and the colour dilation run on the MI355X (e3d_render_cube_map); one scan is
// one call.  Without -o the reference shows the faces in windows; this tool has no display and stops with a message.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "e3d_loader.h"
#include "io_image.h"
#include "io_ply.h"
#include "util.h"

using namespace e3d_host;

int main(int argc, char** argv) {
  std::string cloud_path;
  parse_argument(argc, argv, "-c", cloud_path);
  std::string output_base_path;
  parse_argument(argc, argv, "-o", output_base_path);
  int image_side_length = -1;
  parse_argument(argc, argv, "--size", image_side_length);

  if (cloud_path.empty() || image_side_length <= 0) {
    std::cout << "Please provide the input path and the image side length." << std::endl;
    return EXIT_FAILURE;
  }
  if (output_base_path.empty()) {
    std::cout << "Please provide the output base path (-o): this tool cannot display the faces." << std::endl;
    return EXIT_FAILURE;
  }

  // x, y, z, red, green, blue; an alpha property is ignored, a cloud without colours renders black
  PointCloud cloud;
  if (loadPLYFile(cloud_path, cloud, /*want_rgb=*/true) < 0) {
    std::cout << "Cannot read cloud file: " << cloud_path << "!" << std::endl;
    return EXIT_FAILURE;
  }

  const int size = image_side_length;
  {
    const std::string intrinsics_filename = output_base_path + ".intrinsics.txt";
    std::ofstream intrinsics_stream(intrinsics_filename.c_str(), std::ios::out);
    if (!intrinsics_stream.is_open()) {
      std::cerr << "ERROR: Could not write to " << intrinsics_filename << std::endl;
      return EXIT_FAILURE;
    }
    intrinsics_stream << "# Cube map face image intrinsics in the format: width height fx fy cx cy" << std::endl;
    intrinsics_stream << "# For the principal point the convention having pixel coordinates (0, 0) at the top left corner of the image (instead of the center of the top left pixel) is used." << std::endl;
    intrinsics_stream << size << " " << size << " " << size / 2 << " " << size / 2 << " " << size / 2 << " " << size / 2;
  }

  const size_t n = cloud.size(), face_px = (size_t)size * size;
  std::vector<uint8_t> color(6 * face_px * 3);
  std::vector<float> depth(6 * face_px);
  if (api().e3d_render_cube_map(cloud.xyz.data(), cloud.rgb.data(), n, size, 1, color.data(), depth.data(), nullptr) < 0) {
    std::cerr << "CubeMapRenderer: " << api().e3d_last_error() << std::endl;
    return EXIT_FAILURE;
  }

  const char* face_names[6] = {"front", "left", "back", "right", "down", "up"};
  for (int face = 0; face < 6; ++face) {
    ColorImage img;
    img.width = size; img.height = size;
    img.rgb.assign(color.begin() + face * face_px * 3, color.begin() + (face + 1) * face_px * 3);
    std::string err;
    const std::string image_path = output_base_path + '.' + face_names[face] + ".png";
    if (!imwrite_color(image_path, img, &err)) {
      std::cout << "Error: Cannot write " << image_path << ": " << err << std::endl;
      return EXIT_FAILURE;
    }
    FILE* file = fopen((output_base_path + '.' + face_names[face] + ".depth").c_str(), "wb");
    if (!file) {
      std::cout << "Error: Cannot write depth output file." << std::endl;
      return EXIT_FAILURE;
    }
    const size_t written = fwrite(depth.data() + face * face_px, sizeof(float), face_px, file);
    if (fclose(file) != 0 || written != face_px) {
      std::cout << "Error: Cannot write depth output file." << std::endl;
      return EXIT_FAILURE;
    }
  }

  std::cout << "Finished!" << std::endl;
  return EXIT_SUCCESS;
}
