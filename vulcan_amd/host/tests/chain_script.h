// chain_script.h — the files tests/chain_files.py writes, read back: volumes.txt, script.txt and raw arrays. No GPU and no
// library is needed here: chain_replay.cpp makes the calls, tools/debug/chain_script_parse.cpp runs this parser alone.
//
// A line of script.txt is "<index> <operation> key=value key=value ...", separated by blanks, nothing quoted; a float is the
// hex of its 32 bits, a list is separated by commas, "-" stands for nothing.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace chain
{

struct Error : std::runtime_error
{
  explicit Error(const std::string& text) : std::runtime_error(text) {}
};

inline float HexFloat(const std::string& text)
{
  if (text.empty() || text.size() > 8 || text.find_first_not_of("0123456789abcdefABCDEF") != std::string::npos)
    throw Error("not the hex of a float: '" + text + "'");
  const uint32_t bits = uint32_t(std::stoul(text, nullptr, 16));
  float value;
  std::memcpy(&value, &bits, sizeof(value));
  return value;
}

inline int Integer(const std::string& text)
{
  size_t used = 0;
  int value = 0;
  try { value = std::stoi(text, &used, 10); } catch (const std::exception&) { used = 0; }
  if (text.empty() || used != text.size()) throw Error("not an integer: '" + text + "'");
  return value;
}

inline std::vector<std::string> List(const std::string& text)
{
  std::vector<std::string> out;
  if (text == "-") return out;
  std::istringstream in(text);
  std::string item;
  while (std::getline(in, item, ',')) out.push_back(item);
  return out;
}

struct Step
{
  int index = -1;
  std::string operation;
  std::string text;                                  // the line as written, for messages
  std::map<std::string, std::string> arguments;

  bool Has(const std::string& key) const { return arguments.count(key) != 0; }
  const std::string& Get(const std::string& key) const
  {
    const auto found = arguments.find(key);
    if (found == arguments.end()) throw Error("step " + std::to_string(index) + " (" + operation + ") has no '" + key + "'");
    return found->second;
  }
  int Int(const std::string& key) const { return Integer(Get(key)); }
  bool Flag(const std::string& key) const { return Int(key) != 0; }
  float Float(const std::string& key) const { return HexFloat(Get(key)); }
  std::vector<std::string> Names(const std::string& key) const { return List(Get(key)); }
  bool Nothing(const std::string& key) const { return Get(key) == "-"; }
};

inline Step ParseStep(const std::string& line)
{
  Step step;
  step.text = line;
  std::istringstream in(line);
  std::string index, token;
  if (!(in >> index >> step.operation)) throw Error("a line without an index and an operation: '" + line + "'");
  step.index = Integer(index);
  while (in >> token)
  {
    const size_t at = token.find('=');
    if (at == std::string::npos || at == 0 || at + 1 == token.size() || token.find('=', at + 1) != std::string::npos)
      throw Error("not key=value: '" + token + "' in '" + line + "'");
    if (!step.arguments.emplace(token.substr(0, at), token.substr(at + 1)).second)
      throw Error("a key twice: '" + token + "' in '" + line + "'");
  }
  return step;
}

inline std::vector<Step> ReadScript(const std::string& directory)
{
  std::ifstream in(directory + "/script.txt");
  if (!in.is_open()) throw Error("unable to read " + directory + "/script.txt");
  std::vector<Step> steps;
  std::string line;
  while (std::getline(in, line))
  {
    if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
    steps.push_back(ParseStep(line));
    if (steps.back().index != int(steps.size()) - 1) throw Error("the steps are not numbered in order at '" + line + "'");
  }
  return steps;
}

struct Shape
{
  std::string name;
  int main = 0, excess = 0;
  float voxel_length = 0, truncation_length = 0, depth_min = 0, depth_max = 0;
};

inline std::vector<Shape> ReadVolumes(const std::string& directory)
{
  std::ifstream in(directory + "/volumes.txt");
  if (!in.is_open()) throw Error("unable to read " + directory + "/volumes.txt");
  std::vector<Shape> shapes;
  std::string line;
  while (std::getline(in, line))
  {
    if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
    std::istringstream row(line);
    std::string field[7];
    for (std::string& f : field)
      if (!(row >> f)) throw Error("a volume needs seven fields: '" + line + "'");
    Shape shape;
    shape.name = field[0];
    shape.main = Integer(field[1]);
    shape.excess = Integer(field[2]);
    shape.voxel_length = HexFloat(field[3]);
    shape.truncation_length = HexFloat(field[4]);
    shape.depth_min = HexFloat(field[5]);
    shape.depth_max = HexFloat(field[6]);
    if (shape.main <= 0 || shape.excess < 0) throw Error("a volume without buckets: '" + line + "'");
    shapes.push_back(shape);
  }
  return shapes;
}

// the bytes of a file; `bytes` != 0: exactly that many
inline std::vector<unsigned char> ReadFile(const std::string& path, size_t bytes = 0)
{
  std::ifstream in(path, std::ios::binary | std::ios::ate);
  if (!in.is_open()) throw Error("unable to read " + path);
  const std::streamoff size = in.tellg();
  if (size < 0 || (bytes != 0 && size_t(size) != bytes))
    throw Error(path + " holds " + std::to_string((long long)size) + " bytes, not " + std::to_string(bytes));
  std::vector<unsigned char> data((size_t)size);
  in.seekg(0);
  if (!data.empty() && !in.read(reinterpret_cast<char*>(data.data()), size)) throw Error("short read of " + path);
  return data;
}

inline void WriteFile(const std::string& path, const void* data, size_t bytes)
{
  std::ofstream out(path, std::ios::binary);
  if (!out.is_open()) throw Error("unable to write " + path);
  if (bytes) out.write(static_cast<const char*>(data), (std::streamsize)bytes);
  if (!out) throw Error("short write of " + path);
}

} // namespace chain
