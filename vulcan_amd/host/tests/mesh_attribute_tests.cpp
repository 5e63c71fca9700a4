// mesh_attribute_tests.cpp — per-vertex colours and normals through the C++ class layer -> C ABI -> HIP kernel (no upstream
// case: ref include/vulcan/mesh.h holds points and faces only). The values are held against their CPU statement bit for
// bit by tests/test_gpu_extract_attributes.py; these cases are what a user of the classes sees: Extractor::SetColors /
// SetNormals fill Mesh::colors / Mesh::normals, Exporter writes them, and with both switches off nothing changes.
// Harness: volume_test_support.h.
//
//   ./mesh_attribute_tests            run everything (needs a GPU)
//   ./mesh_attribute_tests <filter>   run the cases whose name contains <filter>
#include <fstream>
#include <sstream>

#include "volume_test_support.h"

// a plane 1.5 m in front of the camera, facing it, in one constant colour, fused once (so every voxel's stored colour is
// the frame's, exactly)
static const Vector3f kColor(0.25f, 0.5f, 0.75f);

static std::shared_ptr<Volume> FusedColouredPlane()
{
  Frame frame;
  frame.depth_projection.SetFocalLength(136, 136);
  frame.depth_projection.SetCenterPoint(80, 60);
  frame.color_projection = frame.depth_projection;
  std::vector<float> depth(size_t(kWidth) * kHeight, 1.5f);
  std::vector<Vector3f> color(size_t(kWidth) * kHeight, kColor);
  frame.depth_image = std::make_shared<Image>(kWidth, kHeight);
  frame.depth_image->CopyFromHost(depth.data());
  frame.color_image = std::make_shared<ColorImage>(kWidth, kHeight);
  frame.color_image->CopyFromHost(color.data());
  auto volume = std::make_shared<Volume>(8192, 2048);
  volume->SetVoxelLength(0.008f);
  for (int i = 0; i < 6; ++i) volume->SetView(frame);
  ColorIntegrator integrator(volume);
  integrator.Integrate(frame);
  return volume;
}

static std::string ReadFile(const std::string& file)
{
  std::ifstream in(file, std::ios::binary);
  std::stringstream text;
  text << in.rdbuf();
  return text.str();
}

TEST(MeshAttributes, ExtractorFillsColorsAndNormals)
{
  auto volume = FusedColouredPlane();
  Extractor extractor(volume);
  extractor.SetAllAllocated(true);
  ASSERT_TRUE(!extractor.GetColors() && !extractor.GetNormals());
  extractor.SetColors(true);
  extractor.SetNormals(true);
  Mesh mesh;
  extractor.Extract(mesh);
  ASSERT_TRUE(mesh.points.size() > 5000 && mesh.faces.size() > 10000);
  ASSERT_EQ(mesh.points.size(), mesh.colors.size());
  ASSERT_EQ(mesh.points.size(), mesh.normals.size());
  for (size_t i = 0; i < mesh.points.size(); ++i)
  {
    // every endpoint holds the frame's colour, and c + t * (c - c) = c
    for (int k = 0; k < 3; ++k) ASSERT_EQ(kColor[k], mesh.colors[i][k]);
    // the distance falls along +z (positive in front of the plane, towards the camera at the origin), so the normal of the
    // positive side is (0, 0, -1); the plane's distance does not depend on x or y
    const Vector3f& n = mesh.normals[i];
    ASSERT_TRUE(std::fabs(n[0]) < 1e-3f && std::fabs(n[1]) < 1e-3f && std::fabs(n[2] + 1.0f) < 1e-3f);
  }

  // one attribute alone, then none: the other members are empty, points and faces stay what they were
  Mesh colours_only;
  extractor.SetNormals(false);
  extractor.Extract(colours_only);
  ASSERT_EQ(mesh.points.size(), colours_only.colors.size());
  ASSERT_TRUE(colours_only.normals.empty());
  Mesh plain;
  extractor.SetColors(false);
  extractor.Extract(plain);
  ASSERT_TRUE(plain.colors.empty() && plain.normals.empty());
  ASSERT_EQ(mesh.points.size(), plain.points.size());
  ASSERT_EQ(mesh.faces.size(), plain.faces.size());
  ASSERT_TRUE(std::memcmp(mesh.points.data(), plain.points.data(), sizeof(Vector3f) * plain.points.size()) == 0);
  ASSERT_TRUE(std::memcmp(mesh.faces.data(), plain.faces.data(), sizeof(Vector3i) * plain.faces.size()) == 0);
  ASSERT_TRUE(std::memcmp(mesh.colors.data(), colours_only.colors.data(), sizeof(Vector3f) * mesh.colors.size()) == 0);

  // the device mesh: buffers of the points' size, or of size 0
  DeviceMesh device;
  extractor.SetNormals(true);
  extractor.Extract(device);
  ASSERT_EQ(device.points.GetSize(), device.normals.GetSize());
  ASSERT_EQ(size_t(0), device.colors.GetSize());
}

TEST(MeshAttributes, ExporterWritesThem)
{
  Mesh mesh;
  mesh.points = { Vector3f(0.1f, -0.25f, 0.35f), Vector3f(1.5f, 2.0f, 0.85f), Vector3f(1e-7f, 123456.789f, 1.35f) };
  mesh.faces = { Vector3i(0, 1, 2) };
  const std::string file = "/tmp/vulcan_mesh_attribute_test.ply";
  Exporter exporter(file);
  exporter.Export(mesh);
  const std::string plain = ReadFile(file);
  ASSERT_TRUE(plain ==
      "ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
      "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 1\n"
      "property list uchar int vertex_indices\nend_header\n"
      "0.1 -0.25 0.35 0 0 0\n1.5 2 0.85 127 127 127\n1e-07 123457 1.35 255 255 255\n3 0 1 2\n");      // as before

  mesh.normals = { Vector3f(0, 0, -1), Vector3f(0.6f, -0.8f, 0), Vector3f(0.57735026f, 0.57735026f, -0.57735026f) };
  mesh.colors = { Vector3f(-0.5f, 0.5f, 2.0f), Vector3f(0.1f, 0.2f, 0.3f), Vector3f(0, 1, 0.998f) };
  exporter.Export(mesh);
  ASSERT_TRUE(ReadFile(file) ==
      "ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
      "property float nx\nproperty float ny\nproperty float nz\n"
      "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 1\n"
      "property list uchar int vertex_indices\nend_header\n"
      "0.1 -0.25 0.35 0 0 -1 0 128 255\n1.5 2 0.85 0.6 -0.8 0 26 51 77\n1e-07 123457 1.35 0.57735 0.57735 -0.57735 0 255 254\n"
      "3 0 1 2\n");

  // attributes of another size are not the mesh's: the file is the plain one
  mesh.normals.pop_back();
  mesh.colors.clear();
  exporter.Export(mesh);
  ASSERT_TRUE(ReadFile(file) == plain);
}

TEST(MeshAttributes, ExtractedMeshExportsWithProperties)
{
  auto volume = FusedColouredPlane();
  Extractor extractor(volume);
  extractor.SetAllAllocated(true);
  Mesh plain, full;
  extractor.Extract(plain);
  extractor.SetColors(true);
  extractor.SetNormals(true);
  extractor.Extract(full);
  const std::string file = "/tmp/vulcan_mesh_attribute_test_plane.ply";
  Exporter exporter(file);
  exporter.Export(plain);
  const std::string before = ReadFile(file);
  ASSERT_TRUE(before.find("property float nx") == std::string::npos);
  exporter.Export(full);
  const std::string after = ReadFile(file);
  ASSERT_TRUE(after.find("property float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty uchar red\n") != std::string::npos);
  ASSERT_TRUE(after.find(" 64 128 191\n") != std::string::npos);          // 0.25, 0.5, 0.75 -> 63.75, 127.5, 191.25 + 0.5, truncated
  ASSERT_TRUE(after.size() > before.size());
  // both switches off again: the bytes of before
  full.colors.clear();
  full.normals.clear();
  exporter.Export(full);
  ASSERT_TRUE(ReadFile(file) == before);
}

int main(int argc, char** argv) { return RunTests("mesh_attribute_tests", argc, argv); }
