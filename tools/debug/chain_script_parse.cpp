// chain_script_parse.cpp — the parser of vulcan_amd/host/tests/chain_script.h alone, for the host's sanitizers: it reads the
// volumes.txt and script.txt that tests/chain_files.py wrote into a directory, every argument of every step through the
// accessor its kind has (a float, an integer, a list, a file that has to exist), and then lines that are NOT well formed, each
// of which has to be refused by an exception and by nothing else. No GPU and no library.
//
//   g++ -std=c++14 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I vulcan_amd/host/tests \
//     tools/debug/chain_script_parse.cpp -o chain_script_parse && ./chain_script_parse DIR
#include <cstdio>
#include <set>

#include "chain_script.h"

static int g_failed = 0;

static void Refused(const char* what, const std::string& line)
{
  try { chain::ParseStep(line); }
  catch (const chain::Error&) { return; }
  std::printf("FAILED: %s was not refused: '%s'\n", what, line.c_str());
  ++g_failed;
}

int main(int argc, char** argv)
{
  if (argc != 2) { std::fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
  const std::string directory = argv[1];
  try
  {
    const std::vector<chain::Shape> shapes = chain::ReadVolumes(directory);
    std::set<std::string> names;
    for (const chain::Shape& shape : shapes)
    {
      names.insert(shape.name);
      std::printf("volume %s (%d, %d) voxel %g truncation %g depth %g .. %g\n", shape.name.c_str(), shape.main, shape.excess,
          shape.voxel_length, shape.truncation_length, shape.depth_min, shape.depth_max);
    }
    const std::vector<chain::Step> steps = chain::ReadScript(directory);
    size_t floats = 0, files = 0, bytes = 0;
    for (const chain::Step& step : steps)
    {
      if (!names.count(step.Get("on"))) throw chain::Error("step " + std::to_string(step.index) + " is on a volume that is not there");
      for (const std::string& name : step.Names("state"))
        if (!names.count(name)) throw chain::Error("a state of a volume that is not there: " + name);
      for (const auto& argument : step.arguments)
      {
        const std::string& key = argument.first;
        const std::string& value = argument.second;
        if (value.size() > 4 && value.compare(value.size() - 4, 4, ".bin") == 0)
        {
          bytes += chain::ReadFile(directory + "/" + value).size();
          ++files;
        }
        else if (key == "r_min" || key == "r_max" || key == "cap" || key == "band" || key == "t_from" || key == "t_max" ||
                 key == "min_abs_distance" || key == "yaw")
        {
          if (!(step.Float(key) == step.Float(key))) throw chain::Error("a NaN in step " + std::to_string(step.index));
          ++floats;
        }
        else if (key == "keep_lo" || key == "keep_hi" || key == "lo" || key == "hi" || key == "origin" || key == "dims")
        {
          for (const std::string& item : step.Names(key)) (void)chain::Integer(item);
        }
        else if (key != "on" && key != "source" && key != "state" && key != "pose")
          (void)step.Int(key);
      }
    }
    std::printf("%zu steps, %zu floats, %zu files of %zu bytes\n", steps.size(), floats, files, bytes);
    if (steps.empty()) { std::printf("FAILED: an empty script\n"); ++g_failed; }
  }
  catch (const std::exception& error)
  {
    std::printf("FAILED: %s\n", error.what());
    ++g_failed;
  }
  Refused("no operation", "7");
  Refused("an index that is no number", "x merge on=map");
  Refused("a token without =", "0 merge on");
  Refused("an empty value", "0 merge on=");
  Refused("an empty key", "0 merge =map");
  Refused("two = in a token", "0 merge on=a=b");
  Refused("a key twice", "0 merge on=map on=other");
  try { (void)chain::HexFloat("3f8000001"); std::printf("FAILED: nine hex digits\n"); ++g_failed; } catch (const chain::Error&) {}
  try { (void)chain::HexFloat("0x3f80"); std::printf("FAILED: a prefix\n"); ++g_failed; } catch (const chain::Error&) {}
  try { (void)chain::Integer("12a"); std::printf("FAILED: 12a\n"); ++g_failed; } catch (const chain::Error&) {}
  try { (void)chain::Integer("99999999999"); std::printf("FAILED: out of range\n"); ++g_failed; } catch (const chain::Error&) {}
  try { (void)chain::ParseStep("3 extract on=map").Get("state"); std::printf("FAILED: a missing key\n"); ++g_failed; } catch (const chain::Error&) {}
  if (chain::HexFloat("3f800000") != 1.0f || chain::HexFloat("bf000000") != -0.5f) { std::printf("FAILED: hex floats\n"); ++g_failed; }
  if (!chain::List("-").empty() || chain::List("a,b").size() != 2) { std::printf("FAILED: lists\n"); ++g_failed; }
  std::printf("chain_script_parse: %d failed\n", g_failed);
  return g_failed ? 1 : 0;
}
