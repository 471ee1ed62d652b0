// boost/filesystem.hpp — STAND-IN written by this project.  TEST INFRASTRUCTURE ONLY; it is not Boost.
//
// The reference's matching/matcher.cpp uses boost::filesystem::path (extension, stem, filename, string, operator<<) and
// directory_iterator (:101-130, :221-233).  std::filesystem has the same interface for all of these, including what is
// observable in the score files: operator<< on a path writes it QUOTED ("dir/name.dat", with " and \ escaped), as Boost does.
// Directory order is the file system's in both; nothing may be compared in directory order, only keyed by file name.
#pragma once
#include <filesystem>

namespace boost {
namespace filesystem = std::filesystem;
}
