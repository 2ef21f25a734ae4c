// Test driver for the sibling reductions of the host layer over fields in their native formats (needs the GPU):
//   ensemble_formats_host_test <in.bin> <outdir>
// in.bin: int32 xs, ys, zs, cs, format (crf_member_format), then cs volumes in that format.  Registers the volumes with
// setFieldData(format), runs an EnsembleMeanCalculator, an EnsembleSpreadCalculator and a SetPredicateCalculator
// (> 0.5, counts 2..20) over them, dumps the three fields (mean.bin, spread.bin, predicate.bin) and prints the format of
// the members the calculators left resident on the device.
#include <cstdio>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "EnsembleCalculators.hpp"
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
    if (raw.size() != 5 * sizeof(int32_t) + n * element * size_t(cs)) throw std::runtime_error("input size does not match its header");
    auto vol = std::make_shared<VolumeData>(xs, ys, zs, 1, cs);
    for (int e = 0; e < cs; e++)
        vol->setFieldData("data", 0, e, native, raw.data() + 5 * sizeof(int32_t) + size_t(e) * n * element);
    auto mean = std::make_shared<EnsembleMeanCalculator>(0);
    auto spread = std::make_shared<EnsembleSpreadCalculator>(0);
    auto predicate = std::make_shared<SetPredicateCalculator>(0);
    vol->addCalculator(mean);
    vol->addCalculator(spread);
    vol->addCalculator(predicate);
    predicate->setSettings(SettingsMap{{"scalar_field_idx", "0"}, {"comparison_operator_type", ">"}, {"comparison_value", "0.5"},
                                       {"count_lower", "2"}, {"count_upper", "20"}});
    vol->updateCalculators();
    const std::shared_ptr<EnsembleReduceCalculator> calcs[3] = {mean, spread, predicate};
    const char* const names[3] = {"/mean.bin", "/spread.bin", "/predicate.bin"};
    for (int i = 0; i < 3; i++) {
        HostCacheEntry entry = vol->getFieldEntryCpu(FieldType::SCALAR, calcs[i]->getOutputFieldName(), 0, 0);
        dump(outDir + names[i], entry->data<float>(), n);
        if (calcs[i]->getResidentMemberFormat() != calcs[0]->getResidentMemberFormat())
            throw std::runtime_error("the calculators disagree about the resident member format");
    }
    std::printf("RESIDENT-FORMAT %d\n", mean->getResidentMemberFormat());
    std::puts("ENSEMBLE-OK");
    return 0;
}

int main(int argc, char** argv) {
    try {
        if (argc >= 3) return run(argv[1], argv[2]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    std::fprintf(stderr, "usage: ensemble_formats_host_test <in.bin> <outdir>\n");
    return 64;
}
