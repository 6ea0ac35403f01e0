// StereoEvaluator -- what the two-view ground truth is for: the disparity maps of a stereo method set against the pairs
// StereoPairCreator writes (<pair>/disp0GT.pfm, +inf = unknown, and <pair>/mask0nocc.png, 255 seen by both cameras, 128
// half-occluded, 0 unknown).  The rules: include/e3d_hip.h, e3d_evaluate_disparity.  The reference has no such tool.
//
//   StereoEvaluator --ground_truth_path DIR --estimates_path DIR [--pairs FILE] [--thresholds 0.5,1,2,4] [--percentiles 50,90,95,99]
//                   [--output_path scores.json] [--error_maps_path DIR] [--timings]
//
// Pairs: the sub-folders of the ground-truth folder that hold disp0GT.pfm, sorted, or the names --pairs lists (one per line, '#'
// starts a comment).  The estimate of a pair is <estimates>/<pair>.pfm if it exists, else <estimates>/<pair>/disp0.pfm; non-finite
// samples are "no estimate".  Every estimate is looked up and its size compared before anything is evaluated.
// stdout: per pair and region (all: mask != 0, nocc: mask == 255) one line of key=value fields -- coverage, avgerr, rms, bad<thr>,
// bad_or_missing<thr>, A<percentile> -- then per region the line "mean" with the mean over the pairs of every derived score.
// The JSON holds the same and the raw counts, sums and quantiles; a NaN is written as null, an infinity as 1e999.
#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "e3d_loader.h"
#include "io_image.h"
#include "io_mlp.h"
#include "io_pfm.h"
#include "util.h"

using namespace e3d_host;

namespace {

constexpr int kMaxThresholds = 8, kMaxPercentiles = 8;
const char* const kRegions[2] = {"all", "nocc"};

// "0.5,1" -> numbers in the order given; false for an empty item or one that is not a number
bool parse_number_list(const std::string& text, std::vector<double>* out) {
  size_t begin = 0;
  while (true) {
    const size_t end = text.find(',', begin);
    const std::string item = text.substr(begin, end == std::string::npos ? std::string::npos : end - begin);
    char* rest = nullptr;
    const double v = strtod(item.c_str(), &rest);
    if (item.empty() || *rest != 0) return false;
    out->push_back(v);
    if (end == std::string::npos) return true;
    begin = end + 1;
  }
}

int fail(const std::string& message) {
  std::cerr << "StereoEvaluator: " << message << std::endl;
  return EXIT_FAILURE;
}

bool exists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0; }

std::string number(double v) {
  if (std::isnan(v)) return "null";
  if (std::isinf(v)) return v > 0 ? "1e999" : "-1e999";
  char buf[64];
  snprintf(buf, sizeof buf, "%.17g", v);
  return buf;
}

template <typename T>
std::string json_list(const T* v, int n) {
  std::string s = "[";
  for (int i = 0; i < n; ++i) s += (i ? ", " : "") + number((double)v[i]);
  return s + "]";
}

std::string short_number(double v) {
  char buf[64];
  snprintf(buf, sizeof buf, "%.9g", v);
  return buf;
}

// rule 7 for one estimate and region
struct Scores {
  double coverage = 0, avgerr = 0, rms = 0, bad[kMaxThresholds] = {0}, bad_or_missing[kMaxThresholds] = {0};
};

Scores derive(const int64_t* counts, const double* sums, int T) {
  Scores s;
  const int64_t n_region = counts[0], n_valid = counts[1];
  if (n_region) s.coverage = (double)n_valid / (double)n_region;
  if (n_valid) { s.avgerr = sums[0] / (double)n_valid; s.rms = std::sqrt(sums[1] / (double)n_valid); }
  for (int t = 0; t < T; ++t) {
    if (n_valid) s.bad[t] = (double)counts[2 + t] / (double)n_valid;
    if (n_region) s.bad_or_missing[t] = (double)(counts[2 + t] + n_region - n_valid) / (double)n_region;
  }
  return s;
}

std::string scores_text(const Scores& s, const std::vector<float>& thr) {
  std::string line = " coverage=" + short_number(s.coverage) + " avgerr=" + short_number(s.avgerr) + " rms=" + short_number(s.rms);
  for (size_t t = 0; t < thr.size(); ++t) line += " bad" + short_number(thr[t]) + "=" + short_number(s.bad[t]);
  for (size_t t = 0; t < thr.size(); ++t) line += " bad_or_missing" + short_number(thr[t]) + "=" + short_number(s.bad_or_missing[t]);
  return line;
}

std::string scores_json(const Scores& s, int T) {
  return "\"coverage\": " + number(s.coverage) + ", \"avgerr\": " + number(s.avgerr) + ", \"rms\": " + number(s.rms) + ", \"bad\": " + json_list(s.bad, T) +
         ", \"bad_or_missing\": " + json_list(s.bad_or_missing, T);
}

struct Pair {
  std::string name, estimate_path;
  int width = 0, height = 0;
};

int run_tool(int argc, char** argv) {
  std::string ground_truth_path, estimates_path, pairs_path, thresholds_text = "0.5,1,2,4", percentiles_text = "50,90,95,99", output_path, error_maps_path;
  parse_argument(argc, argv, "--ground_truth_path", ground_truth_path);
  parse_argument(argc, argv, "--estimates_path", estimates_path);
  parse_argument(argc, argv, "--pairs", pairs_path);
  parse_argument(argc, argv, "--thresholds", thresholds_text);
  parse_argument(argc, argv, "--percentiles", percentiles_text);
  parse_argument(argc, argv, "--output_path", output_path);
  parse_argument(argc, argv, "--error_maps_path", error_maps_path);
  const bool timings = find_argument(argc, argv, "--timings") > 0;

  // every argument and every file name is checked before the library is loaded
  if (ground_truth_path.empty() || estimates_path.empty()) return fail("please provide --ground_truth_path and --estimates_path.");
  std::vector<double> numbers;
  std::vector<float> thresholds;
  bool ok = parse_number_list(thresholds_text, &numbers) && numbers.size() <= (size_t)kMaxThresholds;
  for (size_t i = 0; ok && i < numbers.size(); ++i) {
    thresholds.push_back((float)numbers[i]);
    ok = std::isfinite(thresholds[i]) && thresholds[i] >= 0.f && (i == 0 || thresholds[i] > thresholds[i - 1]);
  }
  if (!ok) return fail("--thresholds must be 1 to 8 numbers >= 0 in strictly ascending order, separated by commas.");
  std::vector<int32_t> percentiles;
  numbers.clear();
  ok = percentiles_text.empty() || (parse_number_list(percentiles_text, &numbers) && numbers.size() <= (size_t)kMaxPercentiles);
  for (size_t i = 0; ok && i < numbers.size(); ++i) {
    ok = numbers[i] >= 1 && numbers[i] <= 100 && numbers[i] == std::floor(numbers[i]);
    percentiles.push_back(ok ? (int32_t)numbers[i] : 0);
  }
  if (!ok) return fail("--percentiles must be at most 8 whole numbers from 1 to 100, separated by commas.");
  const int T = (int)thresholds.size(), P = (int)percentiles.size();

  std::vector<Pair> pairs;
  if (!pairs_path.empty()) {
    std::ifstream f(pairs_path);
    if (!f) return fail("cannot open " + pairs_path);
    std::string line;
    while (std::getline(f, line)) {
      line = line.substr(0, line.find('#'));
      const size_t a = line.find_first_not_of(" \t\r"), b = line.find_last_not_of(" \t\r");
      if (a == std::string::npos) continue;
      Pair p;
      p.name = line.substr(a, b - a + 1);
      pairs.push_back(p);
    }
  } else {
    DIR* dir = opendir(ground_truth_path.c_str());
    if (!dir) return fail("cannot open the folder " + ground_truth_path);
    while (const dirent* entry = readdir(dir)) {
      const std::string name = entry->d_name;
      if (name == "." || name == ".." || !exists(join_path(join_path(ground_truth_path, name), "disp0GT.pfm"))) continue;
      Pair p;
      p.name = name;
      pairs.push_back(p);
    }
    closedir(dir);
    std::sort(pairs.begin(), pairs.end(), [](const Pair& a, const Pair& b) { return a.name < b.name; });
  }
  if (pairs.empty()) return fail("no pair with a disp0GT.pfm in " + ground_truth_path);
  for (Pair& p : pairs) {
    std::string err;
    const PfmImage gt = read_pfm(join_path(join_path(ground_truth_path, p.name), "disp0GT.pfm"), &err, /*header_only=*/true);
    if (gt.width < 1) return fail("pair " + p.name + ": " + err);
    p.width = gt.width; p.height = gt.height;
    p.estimate_path = join_path(estimates_path, p.name + ".pfm");
    if (!exists(p.estimate_path)) p.estimate_path = join_path(join_path(estimates_path, p.name), "disp0.pfm");
    if (!exists(p.estimate_path)) return fail("pair " + p.name + ": no estimate (" + join_path(estimates_path, p.name + ".pfm") + " or " + p.estimate_path + ")");
    const PfmImage est = read_pfm(p.estimate_path, &err, /*header_only=*/true);
    if (est.width < 1) return fail("pair " + p.name + ": " + err);
    if (est.width != p.width || est.height != p.height)
      return fail("pair " + p.name + ": the estimate is " + std::to_string(est.width) + " x " + std::to_string(est.height) + ", the ground truth " +
                  std::to_string(p.width) + " x " + std::to_string(p.height));
  }
  if (!error_maps_path.empty()) create_directories(error_maps_path);

  std::string json = "{\"thresholds\": " + json_list(thresholds.data(), T) + ",\n \"percentiles\": " + json_list(percentiles.data(), P) + ",\n \"pairs\": [";
  Scores mean[2];
  for (size_t k = 0; k < pairs.size(); ++k) {
    const Pair& p = pairs[k];
    std::string err;
    const std::string dir = join_path(ground_truth_path, p.name);
    const PfmImage gt = read_pfm(join_path(dir, "disp0GT.pfm"), &err);
    if (gt.empty()) return fail("pair " + p.name + ": " + err);
    const PfmImage est = read_pfm(p.estimate_path, &err);
    if (est.empty()) return fail("pair " + p.name + ": " + err);
    if (est.width != gt.width || est.height != gt.height) return fail("pair " + p.name + ": the estimate's size differs from the ground truth's");
    GrayImage mask;
    const std::string mask_path = join_path(dir, "mask0nocc.png");
    if (exists(mask_path)) {
      mask = imread_gray(mask_path, &err);
      if (mask.empty()) return fail("pair " + p.name + ": " + err);
      if (mask.width != gt.width || mask.height != gt.height) return fail("pair " + p.name + ": the size of mask0nocc.png differs from the ground truth's");
    }
    ColorImage map;
    if (!error_maps_path.empty()) { map.width = gt.width; map.height = gt.height; map.rgb.resize((size_t)gt.width * gt.height * 3); }

    e3d_disp_eval_t* eval = api().e3d_evaluate_disparity(gt.data.data(), mask.empty() ? nullptr : mask.data.data(), gt.width, gt.height, est.data.data(), 1,
                                                         thresholds.data(), T, P ? percentiles.data() : nullptr, P, map.empty() ? nullptr : map.rgb.data());
    if (!eval) return fail("pair " + p.name + ": " + api().e3d_last_error());
    int64_t counts[2][2 + kMaxThresholds] = {{0}};
    double sums[2][2] = {{0}};
    float quantiles[2 * kMaxPercentiles] = {0};
    std::vector<int64_t> packed_counts(2 * (2 + T));
    int r = api().e3d_disp_eval_get_counts(eval, packed_counts.data());
    if (r >= 0) r = api().e3d_disp_eval_get_sums(eval, &sums[0][0]);
    if (r >= 0) r = api().e3d_disp_eval_get_quantiles(eval, P ? quantiles : nullptr);
    if (timings) {
      float ms[16];
      const char* names[16];
      const int groups = api().e3d_disp_eval_kernel_ms(eval, ms, names, 16);
      for (int g = 0; g < groups && g < 16; ++g) std::cerr << "[timings] " << p.name << " " << names[g] << " " << ms[g] << " ms" << std::endl;
    }
    api().e3d_disp_eval_destroy(eval);
    if (r < 0) return fail("pair " + p.name + ": " + api().e3d_last_error());
    for (int region = 0; region < 2; ++region)
      for (int c = 0; c < 2 + T; ++c) counts[region][c] = packed_counts[region * (2 + T) + c];

    json += std::string(k ? "," : "") + "\n  {\"name\": \"" + p.name + "\", \"width\": " + std::to_string(gt.width) + ", \"height\": " + std::to_string(gt.height) +
            ", \"regions\": {";
    for (int region = 0; region < 2; ++region) {
      const Scores s = derive(counts[region], sums[region], T);
      std::string line = p.name + " " + kRegions[region] + scores_text(s, thresholds);
      for (int q = 0; q < P; ++q) line += " A" + std::to_string(percentiles[q]) + "=" + short_number(quantiles[region * P + q]);
      std::cout << line << std::endl;
      json += std::string(region ? ",\n   " : "\n   ") + "\"" + kRegions[region] + "\": {\"n_region\": " + std::to_string(counts[region][0]) + ", \"n_valid\": " +
              std::to_string(counts[region][1]) + ", \"n_bad\": " + json_list(counts[region] + 2, T) + ", \"sum1\": " + number(sums[region][0]) + ", \"sum2\": " +
              number(sums[region][1]) + ", \"quantiles\": " + json_list(quantiles + region * P, P) + ", " + scores_json(s, T) + "}";
      mean[region].coverage += s.coverage; mean[region].avgerr += s.avgerr; mean[region].rms += s.rms;
      for (int t = 0; t < T; ++t) { mean[region].bad[t] += s.bad[t]; mean[region].bad_or_missing[t] += s.bad_or_missing[t]; }
    }
    json += "}}";
    if (!map.empty() && !imwrite_color(join_path(error_maps_path, p.name + ".png"), map, &err)) return fail("pair " + p.name + ": " + err);
  }
  json += "],\n \"mean\": {";
  const double count = (double)pairs.size();
  for (int region = 0; region < 2; ++region) {
    Scores& m = mean[region];
    m.coverage /= count; m.avgerr /= count; m.rms /= count;
    for (int t = 0; t < T; ++t) { m.bad[t] /= count; m.bad_or_missing[t] /= count; }
    std::cout << "mean " << kRegions[region] << scores_text(m, thresholds) << std::endl;
    json += std::string(region ? ", " : "") + "\"" + kRegions[region] + "\": {" + scores_json(m, T) + "}";
  }
  json += "}}\n";
  if (!output_path.empty()) {
    std::ofstream f(output_path);
    f << json;
    f.close();
    if (!f) return fail("cannot write " + output_path);
  }
  return EXIT_SUCCESS;
}

}  // namespace

int main(int argc, char** argv) { return run_main("StereoEvaluator", run_tool, argc, argv); }
