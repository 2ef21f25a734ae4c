// Test driver for the SEPARATE_SYMMETRIC mode of the host layer over two fields in their native formats (needs the GPU):
//   secondary_formats_host_test <in.bin> <outdir>
// in.bin: int32 xs, ys, zs, cs, format (crf_member_format), then cs volumes of the first field and cs volumes of the second
// field in that format.  Registers both fields with setFieldData(format), runs a CorrelationCalculator in the
// "Separate Symmetric" mode with Pearson (X = the first field, Y = the second), dumps the field (symmetric.bin) and prints
// the formats of the members the calculator left resident on the device.
#include <cstdio>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "CorrelationCalculator.hpp"
#include "VolumeData.hpp"

using namespace crfhost;

static void dump(const std::string& path, const float* v, size_t n) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v), std::streamsize(n * sizeof(float)));
    if (!f) throw std::runtime_error("cannot write " + path);
}

static std::vector<char> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error(std::string("cannot read ") + path);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static int run(const char* inPath, const std::string& outDir) {
    const std::vector<char> raw = slurp(inPath);
    if (raw.size() < 5 * sizeof(int32_t)) throw std::runtime_error("input shorter than its header");
    const int32_t* head = reinterpret_cast<const int32_t*>(raw.data());
    const int xs = head[0], ys = head[1], zs = head[2], cs = head[3], format = head[4];
    const ScalarDataFormat native = format == CRF_MEMBER_U8    ? ScalarDataFormat::BYTE
                                    : format == CRF_MEMBER_U16 ? ScalarDataFormat::SHORT
                                    : format == CRF_MEMBER_F16 ? ScalarDataFormat::FLOAT16
                                                               : ScalarDataFormat::FLOAT;
    const size_t n = size_t(xs) * ys * zs;
    const size_t element = format == CRF_MEMBER_U8 ? 1 : format == CRF_MEMBER_F32 ? 4 : 2;
    if (raw.size() != 5 * sizeof(int32_t) + 2 * n * element * size_t(cs)) throw std::runtime_error("input size does not match its header");
    auto vol = std::make_shared<VolumeData>(xs, ys, zs, 1, cs);
    const char* const names[2] = {"data", "data2"};
    for (int f = 0; f < 2; f++)
        for (int e = 0; e < cs; e++)
            vol->setFieldData(names[f], 0, e, native, raw.data() + 5 * sizeof(int32_t) + (size_t(f) * size_t(cs) + size_t(e)) * n * element);
    auto calc = std::make_shared<CorrelationCalculator>(0);
    vol->addCalculator(calc);
    calc->setSettings(SettingsMap{{"correlation_measure_type", "pearson"}, {"correlation_field_mode", "Separate Symmetric"},
                                  {"scalar_field_idx_ref", "1"}, {"scalar_field_idx_query", "0"}});
    vol->updateCalculators();
    HostCacheEntry entry = vol->getFieldEntryCpu(FieldType::SCALAR, calc->getOutputFieldName(), 0, 0);
    dump(outDir + "/symmetric.bin", entry->data<float>(), n);
    std::printf("RESIDENT-FORMAT %d\n", calc->getResidentMemberFormat());
    std::printf("RESIDENT-SECONDARY-FORMAT %d\n", calc->getResidentSecondaryMemberFormat());
    std::puts("SECONDARY-OK");
    return 0;
}

int main(int argc, char** argv) {
    try {
        if (argc >= 3) return run(argv[1], argv[2]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    std::fprintf(stderr, "usage: secondary_formats_host_test <in.bin> <outdir>\n");
    return 64;
}
