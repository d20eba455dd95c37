/*
 * oracle/shim/fmt/format.h — TEST INFRASTRUCTURE, our own code.
 *
 * The reference's example driver calls fmt::format in two operator<< debug printers
 * (InputData.cpp, OutputData.cpp) that nothing in this project reaches.  This stand-in only
 * lets those files compile: it returns the format string with its arguments ignored.
 */
#pragma once
#include <string>

namespace fmt {
template <class... Args>
std::string format(const char* f, const Args&...) {
  return std::string(f);
}
}  // namespace fmt
