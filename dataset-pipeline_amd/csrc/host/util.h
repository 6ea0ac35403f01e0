// util.h -- command-line and string helpers with the semantics the reference's tools rely on:
// pcl::console::parse_argument ("--flag value" pairs in any order, first occurrence wins, unknown flags ignored)
// and util::SplitStringIntoSet (src/base/util.cc:85-105); the --camera_ids_to_ignore parse and the main() wrapper of the tools.
#pragma once

#include <cstdlib>
#include <cstring>
#include <exception>
#include <iostream>
#include <string>
#include <unordered_set>

namespace e3d_host {

inline int find_argument(int argc, char** argv, const char* name) {
  for (int i = 1; i < argc; ++i)
    if (strcmp(argv[i], name) == 0) return i;
  return -1;
}
inline int parse_argument(int argc, char** argv, const char* name, std::string& val) {
  const int i = find_argument(argc, argv, name) + 1;
  if (i > 0 && i < argc) val = argv[i];
  return i - 1;
}
inline int parse_argument(int argc, char** argv, const char* name, int& val) {
  const int i = find_argument(argc, argv, name) + 1;
  if (i > 0 && i < argc) val = atoi(argv[i]);
  return i - 1;
}
// pcl::console::parse_argument(bool&): true iff atoi(value) == 1
inline int parse_argument(int argc, char** argv, const char* name, bool& val) {
  const int i = find_argument(argc, argv, name) + 1;
  if (i > 0 && i < argc) val = atoi(argv[i]) == 1;
  return i - 1;
}
inline int parse_argument(int argc, char** argv, const char* name, float& val) {
  const int i = find_argument(argc, argv, name) + 1;
  if (i > 0 && i < argc) val = static_cast<float>(atof(argv[i]));
  return i - 1;
}

inline std::unordered_set<std::string> SplitStringIntoSet(char character, const std::string& input) {
  std::unordered_set<std::string> result;
  if (input.empty()) return result;
  std::size_t index = 0;
  while (true) {
    const std::size_t new_index = input.find(character, index);
    result.insert(input.substr(index, (new_index == std::string::npos) ? std::string::npos : (new_index - index)));
    index = new_index + 1;
    if (new_index == std::string::npos || index >= input.size()) break;
  }
  return result;
}

// --camera_ids_to_ignore 3,7 of the tools that read a COLMAP state
inline std::unordered_set<int> parse_camera_ids_to_ignore(int argc, char** argv) {
  std::string list;
  parse_argument(argc, argv, "--camera_ids_to_ignore", list);
  std::unordered_set<int> ids;
  for (const std::string& id : SplitStringIntoSet(',', list)) ids.insert(atoi(id.c_str()));
  return ids;
}

// main() of a tool: library errors (no device, out of memory, ...) arrive as exceptions of the host classes: report, EXIT_FAILURE
inline int run_main(const char* tool_name, int (*run_tool)(int, char**), int argc, char** argv) {
  try {
    return run_tool(argc, argv);
  } catch (const std::exception& e) {
    std::cerr << tool_name << ": " << e.what() << std::endl;
    return EXIT_FAILURE;
  }
}

}  // namespace e3d_host
