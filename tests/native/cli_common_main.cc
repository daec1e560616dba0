// r1cs/cli_common.hpp alone, for a build under ASan and UBSan: cli_common_main <an empty directory>.  Every check is made here;
// the first that fails prints its line and the program exits with status 1, otherwise it prints "ok".
#include <sys/stat.h>

#include "../../circom-witnesscalc_amd/r1cs/cli_common.hpp"

static int failures = 0;
#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            printf("line %d: %s does not hold\n", __LINE__, #x); \
            ++failures;                                           \
        }                                                         \
    } while (0)

static std::string dir;

static int freed = 0;
static void free_int(int* p) {
    ++freed;
    delete p;
}

static std::string put(const char* name, const std::string& text) {
    const std::string path = dir + "/" + name;
    if (!cli::write_file(path.c_str(), text.data(), text.size())) {
        printf("cannot write %s\n", path.c_str());
        exit(1);
    }
    return path;
}

static const std::string MAX = "115792089237316195423570985008687907853269984665640564039457584007913129639935";      // 2^256 - 1
static const std::string TWO256 = "115792089237316195423570985008687907853269984665640564039457584007913129639936";   // 2^256
static const std::string NINES(78, '9');

// the file's outcome: what parse_secret_decimals returns and reports, and an output that only an accepted file touches
static void secrets_case(const std::string& text, size_t n, bool want_ok, size_t want_tokens, size_t want_bad) {
    const std::string path = put("secrets.txt", text);
    uint8_t le[5][32], before[5][32];
    memset(le, 0xa5, sizeof le);
    memcpy(before, le, sizeof le);
    cli::Secrets found;
    const bool ok = cli::parse_secret_decimals(path.c_str(), n, le, found);
    CHECK(ok == want_ok);
    CHECK(found.readable);
    CHECK(found.tokens == want_tokens);
    CHECK(found.bad == want_bad);
    if (!ok) CHECK(memcmp(le, before, sizeof le) == 0);
    if (ok) CHECK(memcmp(le + n, before + n, (5 - n) * 32) == 0);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    dir = argv[1];
    const size_t none = cli::Secrets::none;

    // -- parse_decimal and decimal: round trips at the edges of 256 bits
    uint8_t le[32], zero[32] = {}, ones[32];
    memset(ones, 0xff, sizeof ones);
    memset(le, 0xa5, sizeof le);
    CHECK(cli::parse_decimal("0", 1, le) == cli::Decimal::ok && memcmp(le, zero, 32) == 0 && cli::decimal(le) == "0");
    CHECK(cli::parse_decimal(MAX.data(), MAX.size(), le) == cli::Decimal::ok && memcmp(le, ones, 32) == 0 && cli::decimal(le) == MAX);
    CHECK(cli::parse_decimal(("000" + MAX).data(), MAX.size() + 3, le) == cli::Decimal::ok && cli::decimal(le) == MAX);
    CHECK(cli::parse_decimal("1000000000", 10, le) == cli::Decimal::ok && cli::decimal(le) == "1000000000" && le[0] == 0x00 && le[3] == 0x3b);
    memset(le, 0xa5, sizeof le);
    CHECK(cli::parse_decimal(TWO256.data(), TWO256.size(), le) == cli::Decimal::too_large);
    CHECK(cli::parse_decimal(NINES.data(), NINES.size(), le) == cli::Decimal::too_large);
    CHECK(cli::parse_decimal("", 0, le) == cli::Decimal::not_decimal);
    CHECK(cli::parse_decimal("+1", 2, le) == cli::Decimal::not_decimal);
    CHECK(cli::parse_decimal("12a", 3, le) == cli::Decimal::not_decimal);
    CHECK(cli::parse_decimal((NINES + "x").data(), 79, le) == cli::Decimal::too_large);  // the leftmost character that is wrong decides
    CHECK(cli::parse_decimal(("x" + NINES).data(), 79, le) == cli::Decimal::not_decimal);
    for (int i = 0; i < 32; ++i) CHECK(le[i] == 0xa5);  // a refusal writes nothing

    // -- parse_secret_decimals: the values, each count mismatch, the first bad token, the separators
    secrets_case("0", 1, true, 1, none);
    secrets_case(MAX + "\n", 1, true, 1, none);
    secrets_case(TWO256 + "\n", 1, false, 1, 0);
    secrets_case(NINES, 1, false, 1, 0);
    secrets_case("", 1, false, 0, none);
    secrets_case(" \n\t\r\n", 3, false, 0, none);
    secrets_case("1 2", 3, false, 2, none);
    secrets_case("1 2 3 4", 3, false, 4, none);
    secrets_case("1 2 3", 3, true, 3, none);
    secrets_case("1 2 3 4 5", 5, true, 5, none);
    secrets_case("\t1\r\n\t2\r\n\t3\r\n", 3, true, 3, none);
    secrets_case("1x 2 3", 3, false, 3, 0);
    secrets_case("1 2 3x", 3, false, 3, 2);
    secrets_case("1 +2 3x", 3, false, 3, 1);
    secrets_case("1 2 3 4x", 3, false, 4, none);  // past the wanted ones a token is counted, not read
    secrets_case("1 2x", 3, false, 2, 1);         // too few and a bad one: both are reported, the tool chooses
    secrets_case("1 2 " + TWO256, 3, false, 3, 2);
    {
        uint8_t got[3][32];
        cli::Secrets found;
        CHECK(cli::parse_secret_decimals(put("secrets.txt", "7\n" + MAX + " 1000000000").c_str(), 3, got, found));
        CHECK(cli::decimal(got[0]) == "7" && cli::decimal(got[1]) == MAX && cli::decimal(got[2]) == "1000000000");
        memset(got, 0xa5, sizeof got);
        CHECK(!cli::parse_secret_decimals((dir + "/no_such_file").c_str(), 3, got, found) && !found.readable && found.tokens == 0 && found.bad == none);
        CHECK(got[0][0] == 0xa5 && got[2][31] == 0xa5);
    }

    // -- parse_hex
    std::vector<uint8_t> bytes;
    CHECK(!cli::parse_hex("", 255, bytes));
    CHECK(!cli::parse_hex("a", 255, bytes));
    CHECK(cli::parse_hex("a0", 255, bytes) && bytes == std::vector<uint8_t>{0xa0});
    CHECK(cli::parse_hex("aBcDeF09", 255, bytes) && bytes == (std::vector<uint8_t>{0xab, 0xcd, 0xef, 0x09}));
    CHECK(cli::parse_hex(std::string(510, 'f').c_str(), 255, bytes) && bytes == std::vector<uint8_t>(255, 0xff));
    CHECK(!cli::parse_hex(std::string(512, 'f').c_str(), 255, bytes));
    CHECK(!cli::parse_hex(std::string(511, 'f').c_str(), 255, bytes));
    CHECK(!cli::parse_hex("abcd", 1, bytes) && cli::parse_hex("ab", 1, bytes));
    CHECK(!cli::parse_hex("0x00", 255, bytes) && !cli::parse_hex("0g", 255, bytes) && !cli::parse_hex("00 ", 255, bytes));

    // -- parse_u32
    uint32_t v = 77;
    CHECK(cli::parse_u32("0", 28, v) && v == 0);
    CHECK(cli::parse_u32("28", 28, v) && v == 28);
    CHECK(cli::parse_u32("4294967295", 0xffffffffu, v) && v == 0xffffffffu);
    CHECK(cli::parse_u32("007", 28, v) && v == 7);
    CHECK(cli::parse_u32(" 9", 28, v) && v == 9);  // strtoul's leading space, as the tools always took it
    v = 77;
    CHECK(!cli::parse_u32("29", 28, v) && !cli::parse_u32("4294967296", 0xffffffffu, v) && !cli::parse_u32("99999999999999999999999", 0xffffffffu, v));
    CHECK(!cli::parse_u32("", 28, v) && !cli::parse_u32("1x", 28, v) && !cli::parse_u32("x", 28, v) && !cli::parse_u32("1 ", 28, v));
    CHECK(!cli::parse_u32("-1", 0xffffffffu, v) && !cli::parse_u32("-0", 28, v));
    CHECK(v == 77);  // a refusal writes nothing

    // -- Mapped, read_file and write_file
    {
        cli::Mapped missing, directory, empty, one;
        CHECK(!missing.open((dir + "/no_such_file").c_str()) && missing.data == NULL && missing.len == 0);
        CHECK(!directory.open(dir.c_str()) && directory.data == NULL);
        CHECK(empty.open(put("empty.bin", "").c_str()) && empty.data == NULL && empty.len == 0);
        CHECK(one.open(put("one.bin", "Z").c_str()) && one.len == 1 && one.data != NULL && *(const char*)one.data == 'Z');
    }
    CHECK(!cli::write_file((dir + "/no_such_directory/out.bin").c_str(), "x", 1));
    CHECK(!cli::read_file((dir + "/no_such_file").c_str(), bytes));
    CHECK(cli::read_file((dir + "/empty.bin").c_str(), bytes) && bytes.empty());
    CHECK(cli::read_file(put("three.bin", std::string("a\0b", 3)).c_str(), bytes) && bytes == (std::vector<uint8_t>{'a', 0, 'b'}));

    // -- take_message leaves the status empty; the owner frees once
    {
        gw_status_t st = {OK, strdup("said")};
        CHECK(cli::take_message(st, "fallback") == "said" && st.error_msg == NULL);
        CHECK(cli::take_message(st, "fallback") == "fallback");
        { const cli::Owned<int, free_int> a(new int(1)), nothing(nullptr); }
        CHECK(freed == 1);
        { const cli::Owned<void, free> image(malloc(16)); }
    }

    if (failures) return 1;
    printf("ok\n");
    return 0;
}
