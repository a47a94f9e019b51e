// dcvc - standalone DCVC-UF encoder / decoder for 8- to 16-bit YUV (4:2:0, 4:2:2, 4:4:4, NV12 / P010, Y4M) and 8- to 16-bit RGB pictures on
// an MI355X.
//
// The codec without the research harness: what test_video.py:166-399 (run_one_point_with_stream)
// does around the plugin - read YUV420 frames or RGB pictures, code them picture by picture into the reference's
// stream container, decode the container again, write the reconstruction, log bits and PSNR - as a
// native tool on top of the C ABI only (include/dcvc_amd_codec.h, _ops.h, _stream.h, _image.h). No Python, no
// torch: weights come from a .dcvw file (python -m dcvc_amd.export_weights), pictures travel as u8
// planes and are converted on the device (picture_yuv.hip, rgb_cs.hip).
//
//   dcvc encode --intra I.dcvw [--inter P.dcvw] -i in.yuv -W 1920 -H 1080 [-n frames] --qp-i 32 [--qp-p 32]
//               [--intra-period -1] [--reset-interval 32] [--src-type yuv420|yuv422|yuv444|nv12|p010|nv21|nv16|p210|uyvy|yuy2|y210|v210|rgb24|png|rgb48|png16] [--bit-depth 8|9..16] -o out.bin
//               [--target-bpp B [--qp-min 0] [--qp-max 63] [--rc-horizon 8] [--rc-intra-bonus 0] [--rc-log log.json]
//                [--rc-mode feedback|probe]]
//               [--scene-cut T [--scene-min-gap 8] [--scene-log log.json]] [--scale WxH] [--hash-log hashes.txt]
//               [--target-psnr DB [--qp-min 0] [--qp-max 63]] [--quality-log log.json]
//               [--matrix bt601|bt709|bt2020] [--range full|limited [--yuv-depth 8..16]]
//               [--in-format raw|y4m] [--read-ahead 0..8] [--flush-units 1] [--latency-log log.json]      (-i - | -o -: pipes)
//               [--vbv-maxrate BPP --vbv-bufsize PICTURES [--vbv-init 0.9] [--vbv-log log.json]]
//               [--denoise S[:T] [--denoise-out filtered.yuv] [--denoise-mc R[:LAMBDA] [--mv-log mv.json]]
//                [--grain-log grain.json [--grain-size 0..37] [--grain-window N] [--grain-gain PCT] [--grain-flat F] [--grain-seed N]]]
//               [--deinterlace frame|field[:T] [--field-order tff|bff] [--deinterlace-out progressive.yuv]]
//               [--ivtc film|match[:CTHRESH[:MI[:T]]] [--field-order tff|bff] [--ivtc-out film.yuv] [--ivtc-log log.json]]
//               [--crop auto[:LIMIT[:FRAC[:MINBAR[:N]]]] | --crop WxH+X+Y [--crop-log crop.json] [--crop-out cropped.yuv] [--crop-fill Y:U:V]]
//               [--frame-step 2..8]
//   dcvc decode --intra I.dcvw [--inter P.dcvw] -i out.bin [-o rec.yuv] [-n frames] [--ref in.yuv --json log.json]
//               [--calc-ssim 1] [--verbose-json 1] [--src-type yuv420|yuv422|yuv444|nv12|p010|nv21|nv16|p210|uyvy|yuy2|y210|v210|rgb24|png|rgb48|png16] [--bit-depth 8|9..16] [--out-size WxH]
//               [--fps N:D] [--hash-log hashes.txt] [--verify-hash hashes.txt]
//               [--matrix bt601|bt709|bt2020] [--range full|limited [--yuv-depth 8..16]]
//               [--in-format raw|y4m] [--out-format raw|y4m]                                               (-i - | --ref - | -o -: pipes)
//               [--film-grain grain.json | --grain-strength Y[:C[:SIZE]]]
//               [--uncrop crop.json | --pad SWxSH+X+Y [--pad-fill Y:U:V]]
//               [--interpolate N[:R[:LAMBDA[:LIMIT]]] [--interp-log log.json [--interp-ref clip.yuv]]]
//               Frame-rate conversion. decode --interpolate N (2..8; R 0..15, default 7, and LAMBDA 0..255, default
//               4, are the search's, LIMIT 0..255, default 8, is the selection's: 8-bit code values a sample above which a block
//               repeats the nearer picture; the defaults are untuned) puts N - 1 pictures between every two decoded pictures of
//               one size: n decoded pictures give N (n - 1) + 1 output pictures. The stage keeps a device copy of the previous
//               output picture as the metrics see it (behind --out-size, before grain and pad); when the next one arrives its luma
//               is searched against it once (dcvc_motion_search), then per phase k = 1..N-1 dcvc_interp_select and two
//               dcvc_interp_planes calls (Y; U and V with the format's subsampling) make the picture, which goes through grain,
//               pad, the hashes and -o as a decoded one does, then the decoded picture follows. Hashes and the grain's picture
//               index count output pictures; a -o *.y4m header states N times the rate; --ref, PSNR, MS-SSIM and --json stay those
//               of the decoded pictures; the padding pictures of a ragged chunk do not reach the stage; a change of size restarts
//               it. --interp-log FILE (not "-"): JSON with n, range, lambda, limit, block, width, height and per in-between picture
//               {out_idx, after, k, blocks, fallen, repeated, sum_sad}; one small copy and one wait a picture only with it.
//               --interp-ref FILE (needs the log; raw or Y4M, at the output rate and size): output picture j is measured against
//               its picture j; the log's in-between entries gain psnr_y / psnr_u / psnr_v (before grain and pad), the decoded
//               pictures' entries are read and dropped. The summary line gains ", interpolate xN (K in-between pictures, F
//               repeated)", F from the device's counters, read back once at the end. Planar yuv420 / yuv422 / yuv444 at 8..16 bits;
//               RGB, PNG, wire types, nv12 / p010, --verify-hash and the flags on encode are refused with status 2.
//               encode --frame-step N (2..8): of every N source pictures the first is coded, the others are read and dropped (on a
//               pipe too); the reader does it, in front of every stage, so -n, --crop auto and --read-ahead see the decimated
//               clip and the stream is that of the clip decimated beforehand. Refused with --deinterlace, --ivtc, PNG
//               directories and on decode.
//               Black bars. encode --crop WxH+X+Y codes the window of every source picture; --crop auto finds it:
//               before the first picture is coded N' = min(N, M) of the M source frames the run will read (N 16, 1..256), frames
//               ((2k + 1) M) / (2 N'), are read with pread from the regular -i file (a pipe is refused), uploaded, unpacked when a
//               wire type, measured by dcvc_crop_stats on the luma plane (per row and column the samples above LIMIT, 24, in
//               8-bit code values; the (H + W) * 4 bytes come to the host) and pushed to dcvc_cropdet_*: a row or column is active
//               with more than FRAC / 256 (4) of its samples above the limit, a picture without an active row or column casts no
//               vote, the window is the union of the voting pictures' rectangles, a bar below MINBAR (8) stays and the others are
//               rounded down to multiples of 2 (the chroma grid; the codec takes even sides only) and of 4 vertically with
//               --deinterlace / --ivtc, so content is never cut; untuned defaults. A manual window must lie inside the picture
//               with positive sides on the same grid. The stage sits behind the upload and dcvc_wire_unpack, which land in a
//               buffer of the file's size, and in front of everything else: two dcvc_window_planes calls (Y; U and V) write the
//               window where the upload would have landed - upload -> unpack -> crop -> deinterlace | ivtc -> --scale -> --denoise
//               -> dcvc_pix_to_x - and the run is that of the cropped clip: the parameter set, --batch, the rate and quality
//               flags, --scene-cut, --vbv-*, pipes (manual window), read-ahead and padding pictures see the window's size. A window
//               that is the whole picture issues no launch and gives the file of a run without the flag. yuv420 / yuv422 / yuv444
//               at 8..16 bits, Y4M and the wire types on their 4:2:2 carrier; nv12 / p010 / nv21 and RGB are refused ("sources are
//               not cropped yet"). --crop-out FILE: the cropped pictures in the carrier's raw layout, what decode --ref should be
//               given; --crop-log FILE: JSON - mode, limit, frac, min_bar, source_width / source_height, src_type,
//               chroma_format, bit_depth, probes [{idx, voted, top, bottom, left, right | null}], votes, window {x, y, width,
//               height}, fill [Y, U, V] (limited-range black 16, 128, 128 at the depth, or --crop-fill). One summary line: "crop:
//               auto|manual, WxH+X+Y of SWxSH (V of N' pictures voted)". decode --uncrop FILE (that log) or --pad SWxSH+X+Y:
//               the last stage on the output picture, behind the conversion, --out-size and the grain - the bars carry no grain:
//               two dcvc_window_planes calls with negative offsets write the picture into a buffer of the source's size, the rest
//               at the fill values (--pad-fill Y:U:V over the log's or the default). -o (a Y4M header included), --hash-log and
//               --verify-hash hold the padded picture; --ref, PSNR, --calc-ssim and the JSON log read the unpadded one. Refused
//               with status 2: malformed values, --crop-out / --crop-log / --crop-fill without --crop or named -, a window that
//               does not fit, auto on a pipe, either side's flags on the other; --uncrop with --pad, either without -o or a hash
//               flag, --pad-fill without either, a malformed log, a log of another depth or chroma format, a picture of another
//               size than the log's window or one that does not fit the source, another --src-type ("pictures are not padded yet").
//               Film grain. encode --denoise S[:T] --grain-log FILE: every source picture and the filter's output for
//               it go through dcvc_grain_stats (Y in one call, U and V in one, accumulating on the device; the words come to the
//               host every 8 pictures and at a window's end); per window of --grain-window source pictures (0, the default: the
//               whole clip) dcvc_grain_fit makes a record - seed --grain-seed (1) plus the record's index, size --grain-size (12),
//               tables scaled by --grain-gain percent (100), measured where the filtered picture is flat within --grain-flat (4)
//               code values; untuned defaults - and the records are written as JSON. The stream does not change. decode
//               --film-grain FILE (or --grain-strength: constant tables in sixteenths of an 8-bit code value, SIZE 12, seed 1):
//               behind the conversion and --out-size's resampler every output picture goes through dcvc_grain_apply into a
//               buffer of its own, Y against itself, U and V against the ungrained Y; that buffer is what -o, --hash-log and
//               --verify-hash see - hashes cover the grain - while --ref's metrics and the JSON log read the ungrained picture.
//               The picture index is the output picture's; pictures past the last record keep it. yuv420, yuv422 and yuv444 at
//               8..16 bits. Refused with status 2: --grain-log without --denoise or named -, its options without it or malformed;
//               both decoder flags at once, either without -o or a hash flag, another --src-type ("... pictures are not grained
//               yet"), a malformed file or value, a file of another depth, chroma format or (without --out-size) size, and either
//               side's flags on the other.
//               Pipes: "-" names stdin for -i (and for decode --ref) and stdout for -o; a FIFO, /dev/stdin or any other
//               name that is no regular file (fstat, S_ISREG) works in the same places. Such a source is read front to back and
//               never seeked; a regular file keeps its count up front and every refusal. A name cannot end in .y4m there, so
//               --in-format raw|y4m (encode -i, decode --ref) and --out-format raw|y4m (decode -o) say it; the default is by name.
//               Encoding from a pipe is driven by the end of the input (-n still caps it): the pictures of the last P unit, the
//               padding of a ragged last chunk and a short last --batch follow what was read, and the stream is the regular
//               file's byte for byte. A trailing partial raw picture is dropped with a warning; a Y4M pipe that ends inside a
//               picture ends the run with status 2 after the units of the whole pictures have been written. When -o is a pipe,
//               or with --flush-units 1, encode writes every parameter set and unit as soon as it is complete and keeps only
//               the byte count; decode reads every stream unit by unit (dcvc_stream_next_unit: the units of one codec call plus
//               one of lookahead in memory) and flushes a piped -o after every picture. With -o - every message goes to stderr.
//               SIGPIPE is ignored: a write that fails with EPIPE ends the run with status 1 and one line.
//               --read-ahead N (encode, 0..8; default 0 for a regular -i: the loop as it was; 2 for a pipe): one reader thread
//               fills a ring of N + 1 pinned host slots with read() alone while the main thread codes; the upload leaves from
//               the slot on the one stream, and the slot goes back after the synchronisation behind the conversion. No second
//               stream, no other launch: only the host's read overlaps the coding. The stream does not depend on N.
//               --latency-log FILE (encode): {units: [{type, first_picture, pictures, qp, bytes, read_ms, out_ms}], pictures,
//               bytes}; bytes counts a parameter set in front of the unit, read_ms is when the unit's last source picture was
//               whole in host memory, out_ms when its bytes had been handed to the OS (a regular -o without --flush-units: the
//               one write at the end), both in steady_clock milliseconds since the run started.
//               Refused before a model is loaded: "-" or a non-regular name with --src-type png | png16 (directories), -i -
//               with --ref -, a log named "-", --in-format / --out-format other than raw | y4m or y4m with a type a .y4m name
//               is refused for, --read-ahead outside 0..8, and --read-ahead / --flush-units / --latency-log on decode.
//               --bit-depth (the YUV types; default 8): 9..16 = uint16 little-endian samples (yuv420p10le, ...; 3 H W bytes
//               per picture) for -i (encode), --ref and -o, read and written as DCVC-FM's YUVReader / YUVWriter do
//               (dcvc_pix_to_x / dcvc_x_to_pix with DCVC_PIX_YUV420P: v / max_val, max_val = 2^b - 1; rint(clamp(t max_val))). The
//               stream does not carry it: decode with the depth the source had. PSNR per plane is 10 log10(max_val^2 / mse)
//               over fp32 distortion planes, summed on the device (dcvc_sse_ws), and --calc-ssim uses data_range = max_val;
//               the log has the 8-bit YUV420 log's keys.
//               --src-type (test_video.py's src_type; default yuv420): rgb24 = packed 8-bit RGB pictures back to back in
//               one file (ffmpeg -pix_fmt rgb24 -f rawvideo), -W / -H required to encode; png = -i (encode), --ref and -o
//               are directories of im1.png, im2.png, ... or im00001.png, ... (video_reader.py:10-45; the writer uses
//               im00001.png, ...), the size is taken from the first picture and every picture must have it. RGB is
//               converted with BT.709 on the device (dcvc_rgb_to_x_cs / dcvc_x_to_rgb_cs, test_video.py:55-64, 87-122,
//               366-370); the log then holds the RGB PSNR (dcvc_sse, calc_psnr over 3 H W samples) and, with --calc-ssim,
//               the mean of the three planes' MS-SSIM (calc_msssim_rgb), without _y / _u / _v keys. Both sides must be
//               even, and >= 88 for --calc-ssim.
//               --src-type rgb48 | png16: RGB above 8 bits, everywhere rgb24 / png are (-i, --ref, -o; --batch,
//               --target-bpp, --target-psnr, --quality-log, --scene-cut, --matrix / --range / --yuv-depth, --hash-log /
//               --verify-hash). rgb48 = packed u16 little-endian pictures back to back (ffmpeg -pix_fmt rgb48le -f rawvideo),
//               --bit-depth 9..16 (default 16), values LSB-aligned in 0..2^b - 1, -W / -H required to encode; png16 =
//               directories of 16-bit PNGs under png's naming rules, depth 16 (another --bit-depth is refused, and so is an
//               8-bit file in the directory, with its name). Converted by dcvc_rgb16_to_x_cs / dcvc_x_to_rgb16_cs; the RGB
//               PSNR is 10 log10(max_val^2 / mse) over 3 H W samples (dcvc_sse_ws, the source's planar u16 copy against fp32
//               distortion planes) and --calc-ssim the mean of three dcvc_msssim_range_ws calls with data_range = max_val;
//               the log has the rgb24 log's keys. The manifest carries rgb48 or png16 with one segment of 6 H W bytes.
//               Refused before a model is loaded: --bit-depth 8, --scale / --out-size, names ending in .y4m, odd sides.
//               --src-type yuv422 | yuv444 | nv12 | p010, each with --bit-depth 8|9..16 (p010 = nv12 --bit-depth 10):
//               4:2:2 and 4:4:4 planar pictures (Y, Cb, Cr planes; u16 samples LSB-aligned as yuv4xxp10le) and NV12 (Y, then
//               interleaved Cb Cr rows; above 8 bits the value sits in the high bits, P010 / P012 / P016) for -i (encode),
//               --ref and -o. One picture path at every depth: dcvc_pix_to_x into x or the chunk slot; on decode
//               dcvc_x_to_pix writes fp32 distortion planes and the output samples, PSNR per plane from dcvc_sse_ws (the
//               source's planar samples against those planes, peak = max_val), --calc-ssim from dcvc_msssim_range_ws
//               (every plane's sides >= 88). The log is the YUV420 log: (6 Y + U + V) / 8 for every format,
//               frame_pixel_num = H W. --scale / --out-size are refused for them: not resampled yet.
//               --src-type nv21 | nv16 | p210 | uyvy | yuy2 | y210 | v210: wire formats, the layouts capture cards,
//               cameras and hardware decoders hand over, for -i (encode), --ref and -o. nv21: Y, then Cr Cb pairs (8 bits); nv16:
//               Y, then rows of Cb Cr pairs at full height; uyvy: Cb Y0 Cr Y1 bytes (8 bits); yuy2: Y0 Cb Y1 Cr; v210: 6 pixels in
//               four 32-bit words of three 10-bit fields, rows of 128 ceil(W / 48) bytes (10 bits). nv16 and yuy2 take --bit-depth
//               8|9..16, u16 samples with the value in the high bits above 8 (p210 = nv16 --bit-depth 10, y210 = yuy2 --bit-depth
//               10); another depth than the one a name stands for is refused. Each picture read is unpacked on the device
//               (dcvc_wire_unpack, one launch) into the buffer where a picture of the carrier type - nv12 for nv21, yuv422 for
//               the others - lands, and the run is the carrier type's from there: stream, --batch, --target-bpp, --target-psnr,
//               --quality-log, --scene-cut, metrics and the JSON log are those of the carrier clip, byte for byte. On decode
//               dcvc_x_to_pix writes the carrier picture and dcvc_wire_pack (one launch) the picture -o writes and --hash-log /
//               --verify-hash hash (encode --hash-log too); unused bits, the fields of a v210 group past W and the row padding
//               are zero. The manifest carries nv21, nv16, uyvy, yuy2 or v210, with two segments (Y, the interleaved chroma) for
//               nv21 / nv16 and the whole picture as one for the others. Refused before a model is loaded: --scale / --out-size
//               (not resampled yet), -i / --ref / -o names ending in .y4m, --matrix / --range.
//               A -i, --ref or -o name ending in .y4m is a YUV4MPEG2 file (a file without the magic is refused). Encode:
//               the header supplies -W -H, the source type and the bit depth, flags that disagree are refused; a C420*
//               file takes the yuv420 path (its stream equals the raw file's). Decode: the flags, or - with both absent -
//               the header of --ref *.y4m; -o *.y4m gets a header from the stream's size, the rate from --fps N:D (default:
//               --ref's rate, else 25:1) and FRAME in front of each picture; nv12 / p010 cannot be written as Y4M. A Y4M
//               file that ends inside a picture is refused. Chroma siting is ignored.
//               (the container carries no picture count: the last chunk of an 8-picture model is padded by repeating
//               the final picture, test_video.py:104-110 - give -n, or --ref whose length then trims the output, as the
//               reference's maximum_read = min(g_frame_delay, frame_num - decoded) does)
//               --calc-ssim 1: MS-SSIM of every picture on the GPU (dcvc_msssim; test_video.py:45-51 --calc_ssim), logged as
//               ave_{i,p,all}_frame_msssim{,_y,_u,_v}; needs --ref and both sides >= 176 (chroma planes >= 88).
//               --verbose-json 1: per-picture lists as the reference's --verbose_json writes them (common.py:90-98).
//               --batch N (1..16, default 1): intra pictures N per codec call (dcvc_dmci_compress_batch / _decompress_batch,
//               DESIGN.md 14). Encode: all-intra runs only (no --inter, or --intra-period 1); the file is byte-identical to
//               --batch 1, a short last batch included. Decode: up to N consecutive I units of one size and one qp per call;
//               outputs and log as with --batch 1 (test_time aside).
//               --target-bpp B [--qp-min 0] [--qp-max 63] [--rc-horizon 8] [--rc-intra-bonus 0] [--rc-log log.json] (encode):
//               code to an average of B bits per pixel instead of a constant q_index. All-intra runs (no
//               --inter, or --intra-period 1): every picture gets the largest q_index in [--qp-min, --qp-max] whose
//               predicted stream fits its budget B W H (k + 1) - bits spent (at least a quarter of one picture's share),
//               found by bisection on the size probe (dcvc_dmci_estimate_bits, at most 7 probes), then one compress at
//               that q_index; --qp-i is unused. Runs with an inter model: the one-pass feedback controller
//               (dcvc_amd_rc.h, rate_control.TargetBpp; --qp-i is its start value, I pictures get --rc-intra-bonus steps),
//               no probes - or, with --rc-mode probe, the search below. --qp-p and --batch above 1 are refused with
//               --target-bpp. --rc-log: per coded unit {type, qp, probes, predicted_bytes, bytes} and the totals. The
//               container carries every unit's q_index: decode needs no option.
//               --rc-mode feedback|probe (encode, needs --target-bpp; default feedback = the controller above, byte for byte):
//               probe, with an inter model, bounds every P unit instead of steering the average. A P unit of n existing
//               pictures gets floor(want n) bits, want = max((B W H (pictures coded + horizon) - bits spent) / horizon,
//               B W H / 64) - what the controller steers towards (dcvc_rc_unit_budget_bits) - and the largest q_index in
//               [--qp-min, --qp-max] whose predicted stream fits, searched on the inter model's size probe
//               (dcvc_dmcld_estimate_bits / dcvc_dmcht_estimate_bits: the first stage of compress, the temporal state
//               untouched) from the previous P unit's q_index (--qp-i for the first): gallop, then bisection
//               (dcvc_rc_pick_qp_near; 2 probes when the q_index stays, at most 12). I pictures are not probed: they take
//               that start value plus --rc-intra-bonus, and their bits count as spent. --rc-log: "mode": "probe", P units
//               with probes >= 1 and predicted_bytes, I units with probes 0 and null. All-intra runs ignore the flag (they
//               probe already); the stream format and the decoder do not change.
//               --vbv-maxrate BPP --vbv-bufsize PICTURES [--vbv-init F] [--vbv-log FILE] (encode): a capped rate, on top of
//               any rate mode - constant --qp-i / --qp-p, --target-bpp in both modes, all-intra runs - with LD, HT-S and HT-L, --scene-cut,
//               --scale, pipes, --read-ahead and --flush-units. The decoder-buffer model of dcvc_amd_rc.h (dcvc_rc_vbv_*): r = BPP W H
//               bits arrive per picture period (W H of the coded size), the buffer holds C = PICTURES r bits and starts at F C
//               (default 0.9). A unit - 8 times every byte it adds to the file, --latency-log's bytes - must fit avail = floor(fullness)
//               when its first picture is due; behind it the fullness is min(C, fullness - bits + n r), n = the source pictures it holds
//               (1, 8 for an HT chunk, what the source held for a ragged last chunk). Nothing is padded at the top. Every unit is coded
//               at the q_index its rate mode gives (the modes that search on a budget search on the smaller of theirs and the buffer's)
//               and written when it fits: a P unit then costs one export of the inter codec's state, no probe, and a bucket that never
//               binds leaves the file of the run without the flags. When it does not fit, the state is put back, the largest q_index
//               below whose predicted stream fits is searched on the unit's size probe (dcvc_rc_pick_qp_near from q - 1, down to
//               --qp-min with --target-bpp, else 0) and coded; the coder may exceed the prediction, so the q_index then steps down
//               until the unit fits. At the floor a unit that does not fit is written anyway, with a warning on stderr, and counts as
//               a violation; the exit status stays 0. One summary line: capacity, minimum fullness, units lowered, recodes, violations.
//               --vbv-log: {maxrate_bpp, bufsize_pictures, init, width, height, rate_bits, capacity_bits, units: [{type,
//               first_picture, pictures, qp_mode, qp, probes, recodes, predicted_bytes | null, bytes, fullness_before, fullness_after,
//               violated, underflow_bits}], min_fullness, lowered, recodes, violations}; qp_mode is what the rate mode gave - for a
//               unit whose search was held under the buffer's budget, the largest probed q_index that fits the mode's own budget.
//               --rc-log keeps its keys and reports the final q_index. The stream format and the decoder do not change. Refused before
//               a model is loaded: one of the pair without the other, a value that is not finite or not positive, --vbv-init outside
//               (0, 1], --vbv-init / --vbv-log without the pair, --batch above 1, --target-psnr, a log named "-", any of the flags on
//               decode.
//               --quality-log FILE (encode, any rate mode): the encoder measures every coded unit's reconstruction - an
//               I picture's intra x_hat, a P unit's pictures from dcvc_dmcld_reconstruct / dcvc_dmcht_reconstruct, which leave the
//               temporal state as it is - against the source samples it uploaded (with --scale: the resampled planes, at the coded
//               size), on the device, with the calls and geometry decode --ref uses for the source type and depth (8-bit yuv420:
//               dcvc_x_to_pix(DCVC_PIX_YUV420P, 8) -> dcvc_sse_ws, where the decoder sums fp16 planes on the host: the same values
//               summed in another order). The log: {target_psnr | null, qp_min, qp_max, width, height, src_type, bit_depth, units:
//               [{type, first_picture, pictures, qp, trials, bytes, psnr, frame_psnr, frame_psnr_y, _u, _v (YUV only)}],
//               ave_all_frame_psnr, total_trials}. frame_psnr is the decoder's log's: (6 Y + U + V) / 8, or the RGB PSNR; a unit's
//               psnr is the mean over the pictures it really holds (not the padding pictures of a ragged last chunk). The output
//               file does not change by a byte.
//               --target-psnr DB [--qp-min 0] [--qp-max 63] (encode): every unit is coded at the smallest q_index in the range whose
//               trial coding meets DB (its psnr above >= DB), qp_max when none does: dcvc_rc_pick_qp_for_quality from the previous
//               unit's q_index of the same type (--qp-i for the first of each): gallop, then bisection, 2 trials when the q_index
//               stays, at most 12. An I trial is dcvc_dmci_compress; a P unit's state is exported once, every trial after the first
//               imports it, then compress, reconstruct, measure. The unit is the chosen trial's stream, and the encoder goes on from
//               the state behind that trial (kept from the last trial that met). Picture types, the reset rule and --scene-cut work
//               as without the flag; the container carries every unit's q_index: decode needs no option. Refused: a target that is
//               not finite or not positive, --target-bpp, --qp-p, --batch above 1, --qp-min above --qp-max.
//               --scene-cut T [--scene-min-gap G] [--scene-log log.json] (encode, one-picture inter model = LD): an I picture
//               where the source changes scene. Every source picture is converted first and measured on
//               the device (dcvc_luma_sad: 8-bit luma of x, sum of absolute differences against the previous picture);
//               dcvc_scd_push (dcvc_amd_rc.h) scores it - mafd = 100 sad / (256 W H), score = mafd - the mafd of the last
//               pair that was no cut - and a picture with score >= T (percent of full range; 5 is a reasonable start) at least
//               G (default 8) pictures after the previous I picture is coded as one, on the path of any other I picture.
//               --intra-period and the reset rule stay index-based; with --target-bpp the controller (or the probe mode)
//               sees the final type. --scene-log: {threshold, min_gap, width, height, pictures: [{idx, sad, mafd, score,
//               detected, type, reason: "first" | "period" | "cut" | null}]}. Refused: all-intra runs, --batch above 1, and
//               the 8-picture models (HT-S / HT-L): a P unit there always holds 8 pictures and the container has no picture
//               count, so a chunk cannot be cut short at a scene change. The stream format and the decoder do not change.
//               --scale WxH (encode, yuv420): code the clip at W x H instead of the source's -W x -H. The uploaded
//               u8 / u16 planes are resampled on the device (dcvc_resample_planes, integer Lanczos-3: Y in one call, U and V
//               in one call, every plane on its own with the centre-aligned rule) before dcvc_pix_to_x
//               reads them; the parameter set carries W x H and everything behind - --batch, --target-bpp, --scene-cut -
//               sees a clip of that size. W and H positive and even, each side's ratio in [1/8, 8]; the source size gives
//               the file of a run without the flag. RGB sources are not resampled yet.
//               --denoise S[:T] (encode): a denoising prefilter. S, the spatial strength, and T, the temporal one,
//               are integers in 0..64 in 8-bit code values; one number sets both. Every source picture, once and in source
//               order, goes through dcvc_denoise_planes (Y in one call, U and V in one call) where load_picture leaves it:
//               behind the upload, --scale's resampler and dcvc_wire_unpack, in front of dcvc_pix_to_x. The state is the
//               previous OUTPUT picture at the coded size, in two device buffers used in turn; the conversion and the quality
//               meter read the filter's output buffer where it lies (no copy). Everything behind sees the filtered clip, as
//               with --scale: --batch, --target-bpp, --target-psnr / --quality-log (measured against the filtered samples),
//               --scene-cut, the --vbv-* recodes (which code b.x again: nothing is filtered twice), --read-ahead, pipes and
//               the padding pictures of a ragged last chunk (repeats of the last filtered picture). The stream is the one of a
//               run without the flag on the pre-filtered clip; --denoise 0 gives the file of a run without the flag. For
//               yuv420 / yuv422 / yuv444 at 8..16 bits (.y4m too) and the wire types with a planar 4:2:2 carrier (nv16, p210,
//               uyvy, yuy2, y210, v210: filtered on the carrier); nv12 / p010 / nv21 and the RGB types are refused ("sources
//               are not filtered yet"). --denoise-out FILE (needs --denoise, not "-"): the filtered pictures at the coded size
//               in the carrier type's raw layout and depth, one copy to the host per picture; no padding pictures. One summary
//               line: "denoise: spatial S, temporal T, N pictures filtered". The stream format and the decoder do not change.
//               --denoise-mc R[:LAMBDA] (needs --denoise): the temporal stage reads the previous output picture
//               motion-compensated. R, the search range in half-resolution samples, is an integer in 0..15; LAMBDA, the
//               penalty a sample of vector length, in 0..255 (default 4). Both defaults are untuned: 7 and 4 are the values the
//               design was checked with, nobody has searched for better ones. Per picture with a previous output and T > 0:
//               dcvc_motion_search of the source luma against the previous output's luma, dcvc_motion_compensate_planes of the
//               previous output into a third picture-sized device buffer (Y in one call, U and V in one call with the chroma
//               format's subsampling), and that buffer is dcvc_denoise_planes' prev. The recursive state stays the
//               uncompensated output; the first picture and T == 0 run as without the flag (no launch is added, the stream is
//               the same). --mv-log FILE (needs --denoise-mc, not "-"): JSON with range, lambda, block, width, height and per
//               searched picture {idx, blocks, nonzero, sum_abs_dx, sum_abs_dy, max_abs, sum_sad}; only with it are the
//               vectors copied to the host (one copy and one wait a picture). The summary line gains
//               ", mc range R lambda L (K of B blocks moved)", K counted on the device.
//               --deinterlace MODE[:T] (encode): the source holds woven interlaced frames. MODE frame codes one
//               picture per source frame, field one per field (twice the pictures); T, the motion threshold, is an integer in
//               0..64 in 8-bit code values (default 10; 0: the purely spatial interpolator). --field-order tff | bff (default
//               tff) says which field is the earlier one; a Y4M file with It / Ib supplies it (a flag that disagrees is refused;
//               without --deinterlace such a file is refused as ever). With p0 = 0 for tff, 1 for bff, source frame f gives:
//               frame: picture f = keep p0, woven sample from f itself; field: picture 2f = keep p0, woven sample from frame
//               f - 1, picture 2f + 1 = keep 1 - p0, woven sample from f. Every picture goes through
//               dcvc_deinterlace_planes (Y in one call, U and V in one call) in load_picture: upload -> dcvc_wire_unpack ->
//               deinterlace -> --scale's resampler -> --denoise -> dcvc_pix_to_x. The last two input frames stay on the
//               device in two buffers used in turn; a frame is read once and serves both of its pictures. The filter writes the
//               buffer the next stage reads (no copy). In field mode -n counts coded pictures while the reader and
//               --read-ahead count source frames; a pipe's end ends the clip behind both fields of its last frame.
//               Everything behind sees progressive pictures: --batch, --target-bpp, --target-psnr / --quality-log (measured
//               against the deinterlaced samples), --scene-cut, the --vbv-* recodes, pipes, --latency-log, and the padding
//               pictures of a ragged last chunk (repeats of the last output picture). For yuv420 / yuv422 / yuv444 at 8..16
//               bits (.y4m too) and the wire types with a planar 4:2:2 carrier (nv16, p210, uyvy, yuy2, y210, v210); nv12 /
//               p010 / nv21 and the RGB types are refused ("sources are not deinterlaced yet"). --deinterlace-out FILE (needs
//               --deinterlace, not "-"): the deinterlaced pictures at the SOURCE size (in front of --scale and --denoise) in
//               the carrier type's raw layout and depth: what decode --ref should be given; no padding pictures. One summary
//               line: "deinterlace: MODE, tff|bff, threshold T, N pictures from M frames". The stream format and the decoder
//               do not change.
//               --ivtc MODE[:CTHRESH[:MI[:T]]] (encode): the source is film carried as interlaced video by 3:2
//               pulldown. Every source frame f is measured against f - 1 (dcvc_field_match on the luma planes; the eight words
//               are copied to the host) and pushed (dcvc_ivtc_push): its first field is woven (dcvc_weave_fields, Y in one call,
//               U and V in one) with its own second field (match c) or with the previous frame's (match p, when that fits
//               strictly better); a frame whose chosen match still has a block of more than MI combed samples (video, or a
//               frame whose partner lies outside the clip) goes through dcvc_deinterlace_planes as --deinterlace frame:T does.
//               MODE match codes one picture per frame; MODE film also drops, from every complete cycle of 5 frames counted
//               from frame 0, the frame whose first field differs least from its predecessor's (dcvc_ivtc_drop): 4 (M / 5) +
//               M % 5 pictures from M frames, a ragged last cycle drops nothing. CTHRESH 0..255 (default 9), MI 0..512 (80), T
//               0..64 (10). The stage sits where the deinterlacer does: upload -> dcvc_wire_unpack -> ivtc -> --scale ->
//               --denoise -> dcvc_pix_to_x; the last cycle + 1 source frames stay on the device. -n counts coded pictures, the
//               reader and --read-ahead count source frames (film: whole cycles are read), a pipe's end closes a ragged cycle.
//               --field-order, Y4M It / Ib files and the source types are those of --deinterlace, which --ivtc excludes.
//               --ivtc-out FILE: the pictures at the SOURCE size, as --deinterlace-out; --ivtc-log FILE: JSON, per source frame
//               the eight words, the match, combed and dropped. One summary line: "ivtc: MODE, tff|bff, cthresh C, mi MI,
//               threshold T, N pictures from M frames (P matched to the previous frame, K deinterlaced, D dropped)".
//               --out-size WxH (decode, yuv420): the reconstruction's integer samples (what -o writes at the coded size) are
//               resampled on the device to W x H; -o, --ref (the original clip), PSNR (dcvc_sse_ws on the u8 / u16 output
//               samples against the reference's) and --calc-ssim (dcvc_msssim_range_ws on the same planes) work
//               at that size, frame_pixel_num and the bpp figures count its pixels, and the log gains coded_width and
//               coded_height.
//               --hash-log FILE (decode; encode: all-intra runs) / --verify-hash FILE (decode): picture hashes.
//               Every output picture - the frame_bytes() bytes -o writes or would write, in raw file layout: no Y4M FRAME
//               lines, for png the packed RGB the PNG encodes, with --out-size the resampled picture - is hashed on the
//               device (dcvc_crc32_segments: zlib's CRC-32, one segment per plane - Y, U, V; Y and the interleaved chroma
//               for nv12 / p010; the packed pixels for rgb24 / png), and only the CRC words come to the host: -o and --ref
//               are not needed. A picture's CRC is the combination of its planes' (dcvc_crc32_combine), the sequence CRC
//               that of the pictures': for the raw YUV types and rgb24 it is the crc32 of the whole -o file. Padding pictures
//               of a ragged last chunk and pictures beyond -n are not hashed, as they are not written. The manifest is text:
//                   # dcvc-hash 1 crc32 <src_type> <bit_depth> <width> <height>
//                   <idx> <crc: 8 lowercase hex digits> <plane crc> ...          one line per picture
//                   sequence <crc> <total bytes>
//               --verify-hash compares every picture as it is decoded: the first mismatch prints the picture, the plane,
//               expected and got and ends the run with status 3, as does a manifest with more or fewer pictures than were
//               decoded; a manifest that cannot be read, or whose algorithm, source type, bit depth or size are not the
//               run's, is refused with status 2 before a picture is decoded. encode --hash-log converts the intra encoder's
//               reconstruction with the source's type and depth (at the coded size with --scale) and writes the manifest
//               decode --hash-log writes for that stream with the same type and depth, byte for byte; any --batch. With
//               P pictures the flag is refused: the inter encoders reconstruct no pictures.
//               --matrix bt601|bt709|bt2020, --range full|limited, --yuv-depth B (--src-type rgb24 | png): the
//               colour matrix and the range of the YCbCr picture behind the RGB samples, at every crossing between the two:
//               encode -i, decode -o and --ref (PSNR and --calc-ssim stay between the source's RGB samples and the converted
//               reconstruction), and the pictures --hash-log / --verify-hash hash (encode --hash-log included). limited is
//               Y 16..235, C 16..240 times 2^(B-8) on the scale of B-bit samples, v / (2^B - 1): --yuv-depth (8..16,
//               default 8, only with --range limited) is the depth of the YUV pictures the stream stands for, e.g. 10 to
//               look at a stream coded from yuv420 --bit-depth 10. The defaults, bt709 and full, are the reference's
//               conversion: every run issues dcvc_rgb_to_x_cs / dcvc_x_to_rgb_cs, with bt709 / full when no flag is given, which is
//               what dcvc_rgb_to_x / dcvc_x_to_rgb compute. The stream carries none of
//               this: decode with the flags of the encode, and verify a manifest with the flags it was hashed with. With
//               any of the flags the JSON log gains color_matrix, color_range and color_yuv_depth. Refused: an unknown
//               name, a depth outside 8..16 or without --range limited, and any of the flags with a YUV source type, where
//               nothing is converted. Colour tags in a Y4M header stay ignored.
//
// Picture-type decisions, reset rule, chunk padding, container, PSNR ((6 Y + U + V) / 8 on the
// 0..255 planes) and the JSON log (what compare_bd_rate.py / dcvc_amd/bd_rate.py read) follow
// test_video.py:204-233, 95-110, 240-257, 32-45 and src/utils/common.py:46-116.
#include "dcvc_amd_codec.h"
#include "dcvc_amd_image.h"
#include "dcvc_amd_ops.h"
#include "dcvc_amd_rans.h"
#include "dcvc_amd_rc.h"
#include "stream/container.h"

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <condition_variable>
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <functional>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include <cerrno>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

namespace {

[[noreturn]] void die(const std::string& msg)
{
    fprintf(stderr, "dcvc: %s\n", msg.c_str());
    exit(2);
}

// where the tool's messages go: stdout, or stderr when stdout carries data (-o -)
FILE* g_msg = stdout;

// ------------------------------------------------------------------------------------ pipes
// "-" names stdin (-i, --ref) or stdout (-o); any other name that is no regular file - a FIFO, /dev/stdin - is read and
// written the same way: front to back, never seeking. fstat decides, not an attempt to seek.
bool is_dash(const std::string& p) { return p == "-"; }

bool fd_is_regular(int fd)
{
    struct stat st;
    return fstat(fd, &st) == 0 && S_ISREG(st.st_mode);
}

// a name that exists and is neither a regular file nor a directory, or "-"
bool names_a_pipe(const std::string& p)
{
    if (is_dash(p)) return true;
    struct stat st;
    return stat(p.c_str(), &st) == 0 && !S_ISREG(st.st_mode) && !S_ISDIR(st.st_mode);
}

// a write to a pipe whose reader has gone ends the run with status 1 (SIGPIPE is ignored)
[[noreturn]] void output_closed(const std::string& name)
{
    fprintf(stderr, "dcvc: -o %s: the reader closed the pipe\n", name.c_str());
    exit(1);
}

// every byte, or false with errno set
bool write_all(int fd, const uint8_t* p, size_t n)
{
    while (n > 0) {
        const ssize_t k = write(fd, p, n);
        if (k < 0 && errno == EINTR) continue;
        if (k < 0) return false;
        p += k;
        n -= static_cast<size_t>(k);
    }
    return true;
}

// up to n bytes, short only at the end of the input; -1 on a read error
ssize_t read_upto(int fd, uint8_t* p, size_t n)
{
    size_t got = 0;
    while (got < n) {
        const ssize_t k = read(fd, p + got, n - got);
        if (k < 0 && errno == EINTR) continue;
        if (k < 0) return -1;
        if (k == 0) break;
        got += static_cast<size_t>(k);
    }
    return static_cast<ssize_t>(got);
}

void hip_ok(hipError_t e, const char* what)
{
    if (e != hipSuccess) die(std::string(what) + ": " + hipGetErrorString(e));
}

void abi_ok(long long rc, const char* what)
{
    if (rc < 0) die(std::string(what) + ": " + dcvc_last_error());
}

// ------------------------------------------------------------------------------------ .dcvw
struct WeightFile {
    int kind = -1;                 // 0 dmci, 1 ld, 2 hts, 3 htl
    float skip_thres = 0.f;
    std::vector<char> blob;
    std::vector<std::string> names;
    std::vector<const char*> name_ptrs;
    std::vector<const void*> data;
    std::vector<int> dtypes, ndims;
    std::vector<int64_t> dims;
};

WeightFile load_weights(const std::string& path)
{
    WeightFile w;
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) die("cannot open " + path);
    const std::streamsize size = f.tellg();
    f.seekg(0);
    if (size < 20) die(path + " is not a .dcvw file");
    w.blob.resize(static_cast<size_t>(size));
    if (!f.read(w.blob.data(), size)) die("cannot read " + path);
    const char* p = w.blob.data();
    const char* end = p + size;
    if (std::memcmp(p, "DCVW1\0\0\0", 8) != 0) die(path + " is not a .dcvw file");
    p += 8;
    uint32_t kind, count;
    std::memcpy(&kind, p, 4); std::memcpy(&w.skip_thres, p + 4, 4); std::memcpy(&count, p + 8, 4);
    p += 12;
    w.kind = static_cast<int>(kind);
    // every field is checked against the end of the file before it is read: the file comes from the user
    auto need = [&](uint64_t bytes, const char* what) {
        if (static_cast<uint64_t>(end - p) < bytes) die(path + ": truncated (" + what + ")");
    };
    for (uint32_t i = 0; i < count; ++i) {
        const char* rec = p;
        need(2, "name length");
        uint16_t nl;
        std::memcpy(&nl, p, 2); p += 2;
        need(static_cast<uint64_t>(nl) + 2, "name");
        w.names.emplace_back(p, nl); p += nl;
        const int dtype = static_cast<uint8_t>(p[0]), nd = static_cast<uint8_t>(p[1]); p += 2;
        if (dtype > 2 || nd > 8) die(path + ": bad record " + w.names.back());
        w.dtypes.push_back(dtype); w.ndims.push_back(nd);
        need(8ull * nd + 8, "dimensions");
        uint64_t elems = 1;
        for (int d = 0; d < nd; ++d) {
            int64_t v;
            std::memcpy(&v, p, 8); p += 8;
            if (v < 0 || (v > 0 && elems > (1ull << 40) / static_cast<uint64_t>(v))) die(path + ": bad shape of " + w.names.back());
            elems *= static_cast<uint64_t>(v);
            w.dims.push_back(v);
        }
        uint64_t nbytes;
        std::memcpy(&nbytes, p, 8); p += 8;
        if (nbytes != elems * (dtype == 0 ? 2u : 4u)) die(path + ": size of " + w.names.back() + " does not match its shape");
        need(nbytes, "tensor data");
        w.data.push_back(p);
        p += nbytes;
        const size_t pad = (8 - ((p - rec) & 7)) & 7;
        if (static_cast<size_t>(end - p) < pad && i + 1 < count) die(path + ": truncated (padding)");
        p += std::min<size_t>(pad, static_cast<size_t>(end - p));
    }
    for (const std::string& n : w.names) w.name_ptrs.push_back(n.c_str());
    return w;
}

// the kind field of a .dcvw file's header alone (load_weights checks the rest)
int weight_kind(const std::string& path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) die("cannot open " + path);
    char head[12];
    if (!f.read(head, sizeof(head)) || std::memcmp(head, "DCVW1\0\0\0", 8) != 0) die(path + " is not a .dcvw file");
    uint32_t kind;
    std::memcpy(&kind, head + 8, 4);
    return static_cast<int>(kind);
}

// ------------------------------------------------------------------------------------ codecs
struct Codecs {
    dcvc_dmci* intra = nullptr;
    dcvc_dmcld* ld = nullptr;
    dcvc_dmcht* ht = nullptr;
    int frames_per_p = 1;          // g_frame_delay: 1 (LD), 8 (HT-S / HT-L)
    bool has_inter() const { return ld != nullptr || ht != nullptr; }
};

Codecs make_codecs(const std::string& intra_path, const std::string& inter_path)
{
    Codecs c;
    {
        const WeightFile w = load_weights(intra_path);
        if (w.kind != 0) die(intra_path + " does not hold an intra model");
        c.intra = dcvc_dmci_create();
        if (c.intra == nullptr) die(std::string("cannot create the intra codec: ") + dcvc_last_error());
        abi_ok(dcvc_dmci_set_param(c.intra, static_cast<int>(w.names.size()), w.name_ptrs.data(), w.data.data(),
                                   w.dtypes.data(), w.ndims.data(), w.dims.data(), w.skip_thres), "intra set_param");
    }
    if (!inter_path.empty()) {
        const WeightFile w = load_weights(inter_path);
        const int n = static_cast<int>(w.names.size());
        if (w.kind == 1) {
            c.ld = dcvc_dmcld_create();
            if (c.ld == nullptr) die(std::string("cannot create the inter codec: ") + dcvc_last_error());
            abi_ok(dcvc_dmcld_set_param(c.ld, n, w.name_ptrs.data(), w.data.data(), w.dtypes.data(), w.ndims.data(),
                                        w.dims.data(), w.skip_thres), "inter set_param");
        } else if (w.kind == 2 || w.kind == 3) {
            c.ht = dcvc_dmcht_create(w.kind == 2);
            if (c.ht == nullptr) die(std::string("cannot create the inter codec: ") + dcvc_last_error());
            c.frames_per_p = 8;
            abi_ok(dcvc_dmcht_set_param(c.ht, n, w.name_ptrs.data(), w.data.data(), w.dtypes.data(), w.ndims.data(),
                                        w.dims.data(), w.skip_thres), "inter set_param");
        } else {
            die(inter_path + " does not hold an inter model");
        }
    }
    return c;
}

// ------------------------------------------------------------------------------------ pictures
struct Geometry {
    int H = 0, W = 0, Hp = 0, Wp = 0;      // picture, padded to multiples of 16
    bool rgb = false;                      // RGB pictures (--src-type rgb24 / png: 8 bits; rgb48 / png16: 9..16) instead of YUV420
    int bit_depth = 8;                     // 9..16 = uint16 samples (--bit-depth)
    // --src-type yuv422 / yuv444 / nv12 / p010: a DCVC_PIX_* layout at any depth, with fp32 distortion planes and the metrics
    // on the device at 8 bits too; -1: YUV420 planes (8 bits: fp16 distortion planes, summed on the host) or RGB
    int pix_fmt = -1;
    // RGB: what dcvc_rgb_to_x_cs / dcvc_x_to_rgb_cs are given (--matrix / --range / --yuv-depth; without: BT.709 / full range)
    int matrix = DCVC_MATRIX_BT709, range = DCVC_RANGE_FULL, yuv_depth = 8;
    // --src-type nv21 / nv16 / p210 / uyvy / yuy2 / y210 / v210: the DCVC_WIRE_* layout of the files, beside
    // pix_fmt, its carrier, which everything between dcvc_wire_unpack and dcvc_wire_pack sees; -1: the files hold pix_fmt
    int wire = -1;
    bool pix() const { return pix_fmt >= 0; }
    int yuv_fmt() const { return pix() ? pix_fmt : DCVC_PIX_YUV420P; }      // the layout the conversion calls are given
    bool hbd() const { return bit_depth > 8; }
    bool rgb16() const { return rgb && hbd(); }      // --src-type rgb48 / png16: dcvc_rgb16_to_x_cs / dcvc_x_to_rgb16_cs, fp32 distortion planes
    int Hc() const { return pix_fmt == DCVC_PIX_YUV422P || pix_fmt == DCVC_PIX_YUV444P ? H : H / 2; }      // a chroma plane's sides
    int Wc() const { return pix_fmt == DCVC_PIX_YUV444P ? W : W / 2; }
    size_t y_bytes() const { return static_cast<size_t>(H) * W; }                 // samples of the Y plane
    size_t uv_bytes() const { return static_cast<size_t>(Hc()) * Wc() * 2; }      // samples of the U and V planes
    // one picture: u8 or u16 YUV planes (NV12: interleaved chroma), or packed RGB (planes [3][H][W] on the device), u8 or u16
    size_t frame_bytes() const { return (rgb ? 3 * y_bytes() : y_bytes() + uv_bytes()) * (hbd() ? 2 : 1); }
    // one picture of -i, --ref and -o, and what the hashes cover: frame_bytes(), or the wire format's picture
    size_t file_bytes() const
    {
        if (wire < 0) return frame_bytes();
        const long long n = dcvc_wire_picture_bytes(wire, bit_depth, H, W);
        abi_ok(n, "wire picture");
        return static_cast<size_t>(n);
    }
};

Geometry geometry(int H, int W, bool rgb = false, int bit_depth = 8, int pix_fmt = -1, int wire = -1)
{
    if (rgb && (H <= 0 || W <= 0 || (H & 1) || (W & 1))) {
        die("picture size must be positive and even (RGB pictures are coded as YUV420 is: even sides), got " +
            std::to_string(W) + "x" + std::to_string(H));
    }
    if (H <= 0 || W <= 0 || (H & 1) || (W & 1)) die("picture size must be positive and even (YUV420)");
    Geometry g;
    g.H = H; g.W = W; g.Hp = (H + 15) / 16 * 16; g.Wp = (W + 15) / 16 * 16;
    g.rgb = rgb;
    g.bit_depth = bit_depth;
    g.pix_fmt = pix_fmt;
    g.wire = wire;
    return g;
}

constexpr int kMaxPictureSide = 16384;      // sanity cap for sizes read from a stream (8K is 7680 x 4320)

struct DeviceBuffers {
    uint8_t* yuv8 = nullptr;       // staging for one u8 picture (planes)
    void* x = nullptr;             // fp16 [H][W][3 * frames]
    void* x_hat = nullptr;         // fp16 [frames][Hp][Wp][3]
    void* y16 = nullptr;           // fp16 planes for PSNR (fp32 at a high bit depth)
    uint8_t* out8 = nullptr;       // u8 planes of a reconstruction
    uint8_t* h_yuv = nullptr;      // pinned
    uint16_t* h_p16 = nullptr;     // pinned fp16 planes
    uint8_t* src8 = nullptr;       // u8 planes of the source picture (--calc-ssim)
    double* ssim = nullptr;        // MS-SSIM of Y, U, V (--calc-ssim)
    double* h_ssim = nullptr;      // pinned
    double* sse = nullptr;         // sums of squares of R, G, B or Y, U, V (RGB or high-bit-depth --ref)
    double* h_sse = nullptr;       // pinned
    void* sse_ws = nullptr;        // dcvc_sse_ws's workspace
    long long sse_ws_bytes = 0;
    void* ssim_ws = nullptr;       // dcvc_msssim_range_ws's workspace (the other chroma formats)
    long long ssim_ws_bytes = 0;
    uint8_t* h_src = nullptr;      // pinned: the source picture (RGB or high-bit-depth --ref)
    uint8_t* luma8[2] = {nullptr, nullptr};      // --scene-cut: the 8-bit luma of this picture and of the previous one, in turn
    unsigned long long* sad = nullptr;           // --scene-cut: dcvc_luma_sad's sum
    unsigned long long* h_sad = nullptr;         // pinned
    hipStream_t st = nullptr;
};

DeviceBuffers make_buffers(const Geometry& g, int frames, bool ssim = false, bool scene = false)
{
    DeviceBuffers b;
    hip_ok(hipStreamCreateWithFlags(&b.st, hipStreamNonBlocking), "hipStreamCreate");
    hip_ok(hipMalloc(&b.yuv8, g.frame_bytes()), "hipMalloc");
    hip_ok(hipMalloc(&b.x, static_cast<size_t>(g.H) * g.W * 3 * frames * 2), "hipMalloc");
    hip_ok(hipMalloc(&b.x_hat, static_cast<size_t>(frames) * g.Hp * g.Wp * 3 * 2), "hipMalloc");
    // fp16 planes, or fp32 ones at a high bit depth; the other chroma formats: fp32 planes at every depth
    hip_ok(hipMalloc(&b.y16, g.pix() ? (g.y_bytes() + g.uv_bytes()) * 4 : g.frame_bytes() * 2), "hipMalloc");
    hip_ok(hipMalloc(&b.out8, g.frame_bytes()), "hipMalloc");
    hip_ok(hipHostMalloc(reinterpret_cast<void**>(&b.h_yuv), g.frame_bytes(), hipHostMallocDefault), "hipHostMalloc");
    hip_ok(hipHostMalloc(reinterpret_cast<void**>(&b.h_p16), g.frame_bytes() * 2, hipHostMallocDefault), "hipHostMalloc");
    if (ssim) {
        hip_ok(hipMalloc(&b.src8, g.frame_bytes()), "hipMalloc");
        hip_ok(hipMalloc(&b.ssim, 3 * sizeof(double)), "hipMalloc");
        hip_ok(hipHostMalloc(reinterpret_cast<void**>(&b.h_ssim), 3 * sizeof(double), hipHostMallocDefault), "hipHostMalloc");
    }
    if (g.rgb || g.hbd() || g.pix()) {
        if (!b.src8) hip_ok(hipMalloc(&b.src8, g.frame_bytes()), "hipMalloc");
        hip_ok(hipMalloc(&b.sse, 3 * sizeof(double)), "hipMalloc");
        hip_ok(hipHostMalloc(reinterpret_cast<void**>(&b.h_sse), 3 * sizeof(double), hipHostMallocDefault), "hipHostMalloc");
        hip_ok(hipHostMalloc(reinterpret_cast<void**>(&b.h_src), g.frame_bytes(), hipHostMallocDefault), "hipHostMalloc");
        // RGB: one call over the three planes; YUV420: Y, then U and V, one after the other on the same workspace
        b.sse_ws_bytes = g.rgb ? dcvc_sse_workspace_bytes(3, g.H, g.W)
                               : std::max(dcvc_sse_workspace_bytes(1, g.H, g.W), dcvc_sse_workspace_bytes(2, g.Hc(), g.Wc()));
        hip_ok(hipMalloc(&b.sse_ws, static_cast<size_t>(b.sse_ws_bytes)), "hipMalloc");
    }
    if (ssim && g.rgb16()) {
        // R, G and B one after the other on the same workspace
        b.ssim_ws_bytes = dcvc_msssim_workspace_bytes(1, g.H, g.W);
        hip_ok(hipMalloc(&b.ssim_ws, static_cast<size_t>(b.ssim_ws_bytes)), "hipMalloc");
    }
    if (ssim && g.pix()) {
        b.ssim_ws_bytes = std::max(dcvc_msssim_workspace_bytes(1, g.H, g.W), dcvc_msssim_workspace_bytes(2, g.Hc(), g.Wc()));
        hip_ok(hipMalloc(&b.ssim_ws, static_cast<size_t>(b.ssim_ws_bytes)), "hipMalloc");
    }
    if (scene) {
        for (uint8_t*& p : b.luma8) hip_ok(hipMalloc(&p, g.y_bytes()), "hipMalloc");
        hip_ok(hipMalloc(&b.sad, sizeof(unsigned long long)), "hipMalloc");
        hip_ok(hipHostMalloc(reinterpret_cast<void**>(&b.h_sad), sizeof(unsigned long long), hipHostMallocDefault), "hipHostMalloc");
    }
    return b;
}

void free_buffers(DeviceBuffers& b)
{
    if (b.st) hip_ok(hipStreamSynchronize(b.st), "sync");
    for (void* d : {static_cast<void*>(b.yuv8), b.x, b.x_hat, b.y16, static_cast<void*>(b.out8), static_cast<void*>(b.src8),
                    static_cast<void*>(b.ssim), static_cast<void*>(b.sse), b.sse_ws, b.ssim_ws, static_cast<void*>(b.luma8[0]),
                    static_cast<void*>(b.luma8[1]), static_cast<void*>(b.sad)}) {
        if (d) hip_ok(hipFree(d), "hipFree");
    }
    if (b.h_ssim) hip_ok(hipHostFree(b.h_ssim), "hipHostFree");
    if (b.h_sse) hip_ok(hipHostFree(b.h_sse), "hipHostFree");
    if (b.h_src) hip_ok(hipHostFree(b.h_src), "hipHostFree");
    if (b.h_sad) hip_ok(hipHostFree(b.h_sad), "hipHostFree");
    if (b.h_yuv) hip_ok(hipHostFree(b.h_yuv), "hipHostFree");
    if (b.h_p16) hip_ok(hipHostFree(b.h_p16), "hipHostFree");
    if (b.st) hip_ok(hipStreamDestroy(b.st), "hipStreamDestroy");
    b = DeviceBuffers{};
}

double psnr_plane(const uint8_t* src, const uint16_t* rec16, size_t n)
{
    // metrics.py:10-24 on float64; rec16 holds fp16 values in 0..255
    double se = 0;
    for (size_t i = 0; i < n; ++i) {
        _Float16 h;
        std::memcpy(&h, rec16 + i, 2);
        const double d = static_cast<double>(src[i]) - static_cast<double>(static_cast<float>(h));
        se += d * d;
    }
    const double mse = se / static_cast<double>(n);
    if (std::isnan(mse) || std::isinf(mse)) return -999.9;
    const double p = mse > 1e-10 ? 10.0 * std::log10(255.0 * 255.0 / mse) : 999.9;
    return p < 99.9 ? p : 99.9;
}

// metrics.py:10-24 from the fp64 sum of squared differences over n samples, at the data range `peak`
double psnr_of_sse(double se, double n, double peak = 255.0)
{
    const double mse = se / n;
    if (std::isnan(mse) || std::isinf(mse)) return -999.9;
    const double p = mse > 1e-10 ? 10.0 * std::log10(peak * peak / mse) : 999.9;
    return p < 99.9 ? p : 99.9;
}

// a directory of PNG pictures im1.png, im2.png, ... or im00001.png, ... (video_reader.py:10-45 PNGReader; its naming
// rule: im1.png present -> no padding, else im00001.png present -> 5 digits, else an error)
// the size of a picture of --src-type png16; an 8-bit file is refused with its name
void png16_info(const std::string& p, int& w, int& h)
{
    int depth = 0;
    abi_ok(dcvc_png_info2(p.c_str(), &w, &h, &depth), "png read");
    if (depth != 16) die(p + " is an " + std::to_string(depth) + "-bit PNG: --src-type png16 reads 16-bit pictures (--src-type png reads 8-bit ones)");
}

struct PngDir {
    std::string dir;
    int pad = 5, next = 1;
    std::string path(int n) const
    {
        std::string num = std::to_string(n);
        if (static_cast<int>(num.size()) < pad) num.insert(0, static_cast<size_t>(pad) - num.size(), '0');
        return (std::filesystem::path(dir) / ("im" + num + ".png")).string();
    }
    bool exists(int n) const { return std::filesystem::is_regular_file(path(n)); }
    int count() const
    {
        int n = 0;
        while (exists(n + 1)) ++n;
        return n;
    }
    // the next picture into buf (packed RGB, g.frame_bytes()); false when the sequence has ended
    bool read(uint8_t* buf, const Geometry& g)
    {
        if (!exists(next)) return false;
        const std::string p = path(next++);
        int w = 0, h = 0;
        if (g.rgb16()) png16_info(p, w, h);
        else abi_ok(dcvc_png_info(p.c_str(), &w, &h), "png read");
        if (w != g.W || h != g.H) {
            die(p + " is " + std::to_string(w) + "x" + std::to_string(h) + ", the sequence is " + std::to_string(g.W) + "x" +
                std::to_string(g.H));
        }
        if (g.rgb16()) abi_ok(dcvc_png_read_rgb16(p.c_str(), buf, g.frame_bytes(), &w, &h), "png read");
        else abi_ok(dcvc_png_read_rgb(p.c_str(), buf, g.frame_bytes(), &w, &h), "png read");
        return true;
    }
};

PngDir png_dir(const std::string& dir)
{
    std::error_code ec;
    if (!std::filesystem::is_directory(dir, ec)) die(dir + " is not a directory (--src-type png reads a directory of PNG pictures)");
    PngDir d;
    d.dir = dir;
    d.pad = 1;
    if (d.exists(1)) return d;
    d.pad = 5;
    if (d.exists(1)) return d;
    die(dir + ": unknown image naming convention (im1.png or im00001.png expected)");
}

enum class SrcType { Yuv420, Rgb24, Png, Yuv422, Yuv444, Nv12, Rgb48, Png16 };

bool is_rgb(SrcType t) { return t == SrcType::Rgb24 || t == SrcType::Png || t == SrcType::Rgb48 || t == SrcType::Png16; }
bool is_png(SrcType t) { return t == SrcType::Png || t == SrcType::Png16; }
bool is_rgb_name(const std::string& t) { return t == "rgb24" || t == "png" || t == "rgb48" || t == "png16"; }

// the DCVC_WIRE_* layout a --src-type name stands for (p210 = nv16, y210 = yuy2, both at 10 bits), -1 for the other names
int wire_of(const std::string& s)
{
    return s == "nv21" ? DCVC_WIRE_NV21 : s == "nv16" || s == "p210" ? DCVC_WIRE_NV16 : s == "uyvy" ? DCVC_WIRE_UYVY :
           s == "yuy2" || s == "y210" ? DCVC_WIRE_YUY2 : s == "v210" ? DCVC_WIRE_V210 : -1;
}

const char* wire_name(int wire)
{
    return wire == DCVC_WIRE_NV21 ? "nv21" : wire == DCVC_WIRE_NV16 ? "nv16" : wire == DCVC_WIRE_UYVY ? "uyvy" :
           wire == DCVC_WIRE_YUY2 ? "yuy2" : "v210";
}

// the one depth a wire format's name stands for; 0: the name leaves it to --bit-depth (nv16, yuy2) or is no wire format
int wire_fixed_depth(const std::string& s)
{
    return s == "p210" || s == "y210" || s == "v210" ? 10 : s == "uyvy" || s == "nv21" ? 8 : 0;
}

// a wire format's name gives the type of its carrier: the run is that type's behind dcvc_wire_unpack and up to dcvc_wire_pack
SrcType src_type(const std::string& s)
{
    if (wire_of(s) >= 0) return dcvc_wire_carrier(wire_of(s)) == DCVC_PIX_NV12 ? SrcType::Nv12 : SrcType::Yuv422;
    if (s == "yuv420") return SrcType::Yuv420;
    if (s == "rgb24") return SrcType::Rgb24;
    if (s == "png") return SrcType::Png;
    if (s == "rgb48") return SrcType::Rgb48;
    if (s == "png16") return SrcType::Png16;
    if (s == "yuv422") return SrcType::Yuv422;
    if (s == "yuv444") return SrcType::Yuv444;
    if (s == "nv12" || s == "p010") return SrcType::Nv12;      // p010 = nv12 --bit-depth 10 (bit_depth_arg)
    die("unknown --src-type " + s + " (yuv420, yuv422, yuv444, nv12, p010, nv21, nv16, p210, uyvy, yuy2, y210, v210, rgb24, png, rgb48 or png16)");
}

// the DCVC_PIX_* layout of the types that take the picture path of dcvc_pix_to_x / dcvc_x_to_pix; -1 for the others
int pix_fmt_of(SrcType t)
{
    return t == SrcType::Yuv422 ? DCVC_PIX_YUV422P : t == SrcType::Yuv444 ? DCVC_PIX_YUV444P : t == SrcType::Nv12 ? DCVC_PIX_NV12 : -1;
}

bool is_y4m_name(const std::string& path) { return path.size() >= 4 && path.compare(path.size() - 4, 4, ".y4m") == 0; }

// A file of pictures back to back: raw, or Y4M (a name ending in .y4m, or --in-format y4m: one header line, then a "FRAME...\n"
// line in front of every picture; a file without the magic is refused). Read front to back through a buffer of its own, so
// that stdin ("-"), a FIFO or any other non-regular file serves as well: the reader never seeks. A regular
// file is also counted up front (count), with positioned reads that leave the reader where it is.
struct PictureFile {
    enum Status { Picture, End, Broken };      // Broken: `error` says why (a Y4M source that ends inside a picture, a bad FRAME line)
    int fd = -1;
    std::string path;                          // as the messages name it
    bool y4m = false, regular = true;
    dcvc_y4m_info info{};
    int interlacing = 0;                       // Y4M, open(..., true): 1 for It, 2 for Ib
    std::vector<uint8_t> buf;                  // bytes read ahead of the pictures: header and FRAME lines
    size_t pos = 0, end = 0;
    size_t partial = 0;                        // End: bytes of a trailing partial raw picture
    std::string error;
    // --frame-step N (encode): of every `step` pictures the first is a picture of this file, the others are read
    // and dropped: count, offsets and next see the decimated clip, and so does everything behind them
    int step = 1;
    long long served = 0;                      // pictures next has handed out
    // format: "" = by name, "raw" or "y4m" (--in-format); interlaced: a Y4M file may say It or Ib (--deinterlace)
    void open(const std::string& p, const std::string& format = "", bool interlaced = false)
    {
        path = is_dash(p) ? "stdin" : p;
        fd = is_dash(p) ? 0 : ::open(p.c_str(), O_RDONLY);
        if (fd < 0) die("cannot open " + p);
        regular = fd_is_regular(fd);
        buf.resize(1024);
        y4m = format.empty() ? is_y4m_name(p) : format == "y4m";
        if (!y4m) return;
        const size_t n = fill_line();
        const int rc = interlaced ? dcvc_y4m_parse_header_i(buf.data() + pos, n, &info, &interlacing) : dcvc_y4m_parse_header(buf.data() + pos, n, &info);
        if (rc < 0) die(path + " is no Y4M file: " + dcvc_last_error());
        pos += static_cast<size_t>(info.header_bytes);
    }
    // reads until the buffer holds a whole line, 1024 bytes or the end of the input; the bytes it holds
    size_t fill_line()
    {
        if (pos > 0) {
            std::memmove(buf.data(), buf.data() + pos, end - pos);
            end -= pos;
            pos = 0;
        }
        size_t scanned = 0;
        for (;;) {
            if (std::memchr(buf.data() + scanned, '\n', end - scanned) != nullptr || end == buf.size()) return end;
            scanned = end;
            ssize_t k;
            do k = ::read(fd, buf.data() + end, buf.size() - end); while (k < 0 && errno == EINTR);
            if (k <= 0) return end;
            end += static_cast<size_t>(k);
        }
    }
    // pictures in a regular file; a Y4M file that ends inside a picture is refused. The reader's position is not touched.
    long long count(size_t frame_bytes)
    {
        struct stat st;
        if (fstat(fd, &st) != 0) die("cannot read " + path);
        const long long size = st.st_size;
        if (!y4m) return (size / static_cast<long long>(frame_bytes) + step - 1) / step;
        long long n = 0, at = info.header_bytes;
        char line[1024];
        for (;;) {
            const ssize_t got = pread(fd, line, sizeof(line), at);
            if (got <= 0) return (n + step - 1) / step;
            const int len = dcvc_y4m_frame_header_bytes(line, static_cast<size_t>(got));
            if (len < 0) die(path + ": no FRAME line where a picture should start (" + dcvc_last_error() + ")");
            at += len;
            if (at + static_cast<long long>(frame_bytes) > size) {
                die(path + " ends inside picture " + std::to_string(n + 1) + " (" + std::to_string(frame_bytes) + " bytes each)");
            }
            at += static_cast<long long>(frame_bytes);
            ++n;
        }
    }
    // where the first n pictures of a regular file start (--crop auto reads some of them with pread); the reader's position is
    // not touched
    std::vector<long long> offsets(size_t frame_bytes, long long n)
    {
        std::vector<long long> at_of;
        long long at = y4m ? info.header_bytes : 0;
        char line[1024];
        for (long long i = 0; i < (n - 1) * step + 1; ++i) {
            if (y4m) {
                const ssize_t got = pread(fd, line, sizeof(line), at);
                const int len = got <= 0 ? -1 : dcvc_y4m_frame_header_bytes(line, static_cast<size_t>(got));
                if (len < 0) die(path + ": no FRAME line where picture " + std::to_string(i + 1) + " should start");
                at += len;
            }
            if (i % step == 0) at_of.push_back(at);
            at += static_cast<long long>(frame_bytes);
        }
        return at_of;
    }
    // the next picture. Calls nothing that dies and nothing from HIP: the read-ahead thread runs it.
    Status next(uint8_t* dst, size_t frame_bytes)
    {
        // the pictures between two that are kept pass through dst: a pipe is read, never skipped
        for (int k = 1; k < step && served > 0; ++k) {
            const Status s = next_of_file(dst, frame_bytes);
            if (s != Picture) return s;
        }
        const Status s = next_of_file(dst, frame_bytes);
        if (s == Picture) ++served;
        return s;
    }
    Status next_of_file(uint8_t* dst, size_t frame_bytes)
    {
        if (y4m) {
            const size_t n = fill_line();
            if (n == 0) return End;
            const int len = dcvc_y4m_frame_header_bytes(buf.data(), n);
            if (len < 0) {
                error = path + ": no FRAME line where a picture should start (" + dcvc_last_error() + ")";
                return Broken;
            }
            pos += static_cast<size_t>(len);
        }
        size_t got = std::min(end - pos, frame_bytes);
        std::memcpy(dst, buf.data() + pos, got);
        pos += got;
        if (got < frame_bytes) {
            const ssize_t k = read_upto(fd, dst + got, frame_bytes - got);
            if (k < 0) {
                error = "cannot read " + path + ": " + strerror(errno);
                return Broken;
            }
            got += static_cast<size_t>(k);
        }
        if (got == frame_bytes) return Picture;
        if (y4m) {
            error = path + " ends inside a picture";
            return Broken;
        }
        partial = got;
        return End;
    }
    // the next picture; false when the file has ended (a Y4M file inside a picture: refused)
    bool read(uint8_t* dst, size_t frame_bytes)
    {
        const Status s = next(dst, frame_bytes);
        if (s == Broken) die(error);
        return s == Picture;
    }
    void close()
    {
        if (fd > 0) ::close(fd);
        fd = -1;
    }
};

// what a Y4M header says against the flags: explicit -W / -H / --src-type / --bit-depth that disagree are refused
struct Y4mSource {
    SrcType type = SrcType::Yuv420;
    int depth = 8;
};

struct Args;
Y4mSource y4m_source(const PictureFile& pf, const Args& a, bool check_size);

// a JSON number as Python's json.dump writes it: NaN and the infinities as NaN / Infinity / -Infinity, else 17 digits
std::string jnum(double v)
{
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v > 0 ? "Infinity" : "-Infinity";
    char buf[32];
    snprintf(buf, sizeof(buf), "%.17g", v);
    return buf;
}

std::string jlist(const std::vector<double>& v)
{
    std::string s = "[";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + jnum(v[i]);
    return s + "]";
}

struct Args {
    std::map<std::string, std::string> kv;
    bool has(const std::string& k) const { return kv.count(k) != 0; }
    std::string str(const std::string& k, const std::string& def = "") const { return has(k) ? kv.at(k) : def; }
    int num(const std::string& k, int def) const { return has(k) ? atoi(kv.at(k).c_str()) : def; }
};

Args parse(int argc, char** argv)
{
    Args a;
    for (int i = 2; i < argc; ++i) {
        std::string k = argv[i];
        if (k.rfind("-", 0) != 0 || i + 1 >= argc) die("bad argument " + k);
        while (!k.empty() && k[0] == '-') k.erase(0, 1);
        a.kv[k] = argv[++i];
    }
    return a;
}

// test_video.py:204-213
bool is_intra_picture(int idx, int intra_period)
{
    if (idx == 0 || intra_period == 1) return true;
    return intra_period > 1 && idx != 1 && idx % intra_period == 1;
}

// --bit-depth: 8 (the default, u8 samples) or 9..16 (u16 samples), YUV sources only; --src-type p010 is nv12 at 10 bits
int bit_depth_arg(const Args& a, SrcType type)
{
    const bool p010 = a.str("src-type") == "p010";
    // the wire formats with one depth: p210, y210 and v210 hold 10-bit samples, uyvy and nv21 8-bit ones
    const int fixed = wire_fixed_depth(a.str("src-type"));
    if (!a.has("bit-depth")) return p010 ? 10 : fixed ? fixed : type == SrcType::Rgb48 || type == SrcType::Png16 ? 16 : 8;
    const std::string s = a.str("bit-depth");
    if (type == SrcType::Rgb48 || type == SrcType::Png16) {
        char* e16 = nullptr;
        const long v16 = strtol(s.c_str(), &e16, 10);
        const bool number = !s.empty() && *e16 == '\0';
        if (type == SrcType::Png16 && (!number || v16 != 16)) die("--src-type png16 holds 16-bit samples: --bit-depth " + s + " disagrees");
        if (!number || v16 < 9 || v16 > 16) die("--src-type rgb48 takes --bit-depth 9..16 (8-bit RGB pictures are --src-type rgb24), got " + s);
        return static_cast<int>(v16);
    }
    if (type == SrcType::Rgb24 || type == SrcType::Png) die("--bit-depth is for --src-type yuv420 only (RGB sources are 8-bit)");
    char* end = nullptr;
    const long v = strtol(s.c_str(), &end, 10);
    if (s.empty() || *end != '\0' || v < 8 || v > 16) die("--bit-depth must be 8 or 9..16, got " + s);
    if (p010 && v != 10) die("--src-type p010 is nv12 at 10 bits: --bit-depth " + s + " disagrees (use --src-type nv12 --bit-depth " + s + ")");
    if (fixed && v != fixed) {
        const std::string t = a.str("src-type");
        if (t == "p210" || t == "y210") {
            const std::string base = t == "p210" ? "nv16" : "yuy2";
            die("--src-type " + t + " is " + base + " at 10 bits: --bit-depth " + s + " disagrees (use --src-type " + base + " --bit-depth " + s + ")");
        }
        die("--src-type " + t + " holds " + std::to_string(fixed) + "-bit samples: --bit-depth " + s + " disagrees");
    }
    return static_cast<int>(v);
}

const char* src_type_name(SrcType t)
{
    return t == SrcType::Yuv420 ? "yuv420" : t == SrcType::Yuv422 ? "yuv422" : t == SrcType::Yuv444 ? "yuv444" : t == SrcType::Nv12 ? "nv12" :
           t == SrcType::Rgb24 ? "rgb24" : t == SrcType::Rgb48 ? "rgb48" : t == SrcType::Png16 ? "png16" : "png";
}

// --src-type nv21 | nv16 | p210 | uyvy | yuy2 | y210 | v210: the DCVC_WIRE_* layout of the run's files, -1 for the other types.
// What the flags alone decide is refused before a model is loaded: a depth the format does not have, and Y4M files.
int wire_arg(const Args& a, bool encoding)
{
    const std::string t = a.str("src-type");
    const int wire = wire_of(t);
    if (wire < 0) return -1;
    bit_depth_arg(a, src_type(t));
    for (const char* k : {"i", "ref", "o"}) {
        if ((std::strcmp(k, "i") != 0 || encoding) && a.has(k) && is_y4m_name(a.str(k))) {
            die(std::string(k[0] == 'r' ? "--" : "-") + k + " " + a.str(k) + ": Y4M has no tag for --src-type " + t + "; use a raw file");
        }
    }
    return wire;
}

// --src-type rgb48 | png16: what the flags alone decide is refused before a model is loaded: the depth, Y4M names, odd sizes
void rgb16_arg(const Args& a, bool encoding)
{
    const std::string t = a.str("src-type");
    if (t != "rgb48" && t != "png16") return;
    bit_depth_arg(a, src_type(t));
    for (const char* k : {"i", "ref", "o"}) {
        if ((std::strcmp(k, "i") != 0 || encoding) && a.has(k) && is_y4m_name(a.str(k))) {
            die(std::string(k[0] == 'r' ? "--" : "-") + k + " " + a.str(k) + ": a Y4M file holds YUV pictures, not --src-type " + t);
        }
    }
}

// the file's pictures of a wire format, beside the carrier pictures in DeviceBuffers: one launch converts each way
struct WireStage {
    uint8_t* in = nullptr;         // a picture of -i or --ref, in front of dcvc_wire_unpack
    uint8_t* h_in = nullptr;       // pinned
    uint8_t* out = nullptr;        // dcvc_wire_pack's picture: what -o writes and the hashes cover
    uint8_t* h_out = nullptr;      // pinned
    void create(const Geometry& g)
    {
        destroy();                 // a stream may switch parameter sets
        if (g.wire < 0) return;
        hip_ok(hipMalloc(&in, g.file_bytes()), "hipMalloc");
        hip_ok(hipMalloc(&out, g.file_bytes()), "hipMalloc");
        hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_in), g.file_bytes(), hipHostMallocDefault), "hipHostMalloc");
        hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_out), g.file_bytes(), hipHostMallocDefault), "hipHostMalloc");
    }
    // the picture in h_in (or in `from`, a read-ahead slot) -> `carrier`, where an upload of the carrier type's picture lands
    void upload(const Geometry& g, uint8_t* carrier, hipStream_t st, const uint8_t* from = nullptr) const
    {
        hip_ok(hipMemcpyAsync(in, from ? from : h_in, g.file_bytes(), hipMemcpyHostToDevice, st), "H2D");
        abi_ok(dcvc_wire_unpack(in, g.wire, g.bit_depth, g.H, g.W, carrier, st), "wire_unpack");
    }
    // the carrier picture dcvc_x_to_pix wrote -> out
    void pack(const Geometry& g, const uint8_t* carrier, hipStream_t st) const
    {
        abi_ok(dcvc_wire_pack(carrier, g.wire, g.bit_depth, g.H, g.W, out, st), "wire_pack");
    }
    void destroy()
    {
        for (uint8_t* d : {in, out}) {
            if (d) hip_ok(hipFree(d), "hipFree");
        }
        for (uint8_t* h : {h_in, h_out}) {
            if (h) hip_ok(hipHostFree(h), "hipHostFree");
        }
        *this = WireStage{};
    }
};

Y4mSource y4m_source(const PictureFile& pf, const Args& a, bool check_size)
{
    Y4mSource y;
    y.type = pf.info.pix_fmt == DCVC_PIX_YUV422P ? SrcType::Yuv422 : pf.info.pix_fmt == DCVC_PIX_YUV444P ? SrcType::Yuv444 : SrcType::Yuv420;
    y.depth = pf.info.bit_depth;
    const std::string what = pf.path + " holds " + std::to_string(pf.info.width) + "x" + std::to_string(pf.info.height) + " " +
                             src_type_name(y.type) + " pictures of " + std::to_string(y.depth) + " bits";
    if (check_size && ((a.has("W") && a.num("W", 0) != pf.info.width) || (a.has("H") && a.num("H", 0) != pf.info.height))) {
        die(what + ", not the -W x -H given");
    }
    if (a.has("src-type") && src_type(a.str("src-type")) != y.type) die(what + ", not --src-type " + a.str("src-type"));
    if ((a.has("bit-depth") || a.str("src-type") == "p010") && bit_depth_arg(a, y.type) != y.depth) die(what + ", not the --bit-depth given");
    return y;
}

// --fps N:D (decode, -o *.y4m): the rate the Y4M header states
bool fps_arg(const Args& a, int& num, int& den)
{
    if (!a.has("fps")) return false;
    const std::string s = a.str("fps");
    const size_t c = s.find(':');
    const std::string part[2] = {s.substr(0, c), c == std::string::npos ? std::string() : s.substr(c + 1)};
    for (const std::string& p : part) {
        if (p.empty() || p.size() > 9 || p.find_first_not_of("0123456789") != std::string::npos || atoi(p.c_str()) <= 0) {
            die("--fps must be N:D with two positive numbers, got " + s);
        }
    }
    num = atoi(part[0].c_str()); den = atoi(part[1].c_str());
    return true;
}

// --batch: 1 (the default) .. 16 pictures per intra call; refused before anything touches the device
int batch_arg(const Args& a)
{
    if (!a.has("batch")) return 1;
    const std::string s = a.str("batch");
    char* end = nullptr;
    const long v = strtol(s.c_str(), &end, 10);
    if (s.empty() || *end != '\0' || v < 1 || v > 16) die("--batch must be in 1..16, got " + s);
    return static_cast<int>(v);
}

// --target-bpp and its companions, refused before anything touches the device
struct RateArgs {
    bool on = false;
    double target_bpp = 0;
    int qp_min = 0, qp_max = 63, horizon = 8, intra_bonus = 0;
    std::string log;
    bool probe = false;      // --rc-mode probe: P units searched on the inter model's size probe
};

int int_arg(const Args& a, const std::string& key, int def, int lo, int hi)
{
    if (!a.has(key)) return def;
    const std::string s = a.str(key);
    char* end = nullptr;
    const long v = strtol(s.c_str(), &end, 10);
    if (s.empty() || *end != '\0' || v < lo || v > hi) {
        die("--" + key + " must be in " + std::to_string(lo) + ".." + std::to_string(hi) + ", got " + s);
    }
    return static_cast<int>(v);
}

// -i / --ref / -o on pipes, --in-format / --out-format, --read-ahead, --flush-units, --latency-log: what the
// flags alone decide is refused before a model is loaded
struct PipeArgs {
    std::string in_format, out_format;      // "" = by name, "raw" or "y4m"
    int read_ahead = 0;                     // encode: pinned slots filled ahead of the coder by a reader thread; 0: today's loop
    bool flush_units = false;               // encode: every unit is written and flushed as soon as it is complete
    std::string latency_log;
    bool in_is_y4m(const std::string& name) const { return in_format.empty() ? is_y4m_name(name) : in_format == "y4m"; }
    bool out_is_y4m(const std::string& name) const { return out_format.empty() ? is_y4m_name(name) : out_format == "y4m"; }
};

PipeArgs pipe_args(const Args& a, bool encoding)
{
    PipeArgs p;
    const std::string t = a.str("src-type", "yuv420");
    for (const char* k : {"in-format", "out-format"}) {
        if (!a.has(k)) continue;
        const std::string v = a.str(k), flag = std::string("--") + k;
        if (v != "raw" && v != "y4m") die(flag + " must be raw or y4m, got " + v);
        if (encoding && k[0] == 'o') die("--out-format is a decoder flag: it names the format of the pictures -o writes");
        if (v != "y4m") continue;
        // the types a name ending in .y4m is refused for, in that path's words
        if (wire_of(t) >= 0) die(flag + " y4m: Y4M has no tag for --src-type " + t + "; use a raw file");
        if (t == "nv12" || t == "p010") die(flag + " y4m: Y4M has no tag for interleaved chroma (--src-type " + t + "); use a raw file");
        if (is_rgb_name(t)) die(flag + " y4m: a Y4M file holds YUV pictures, not --src-type " + t);
    }
    p.in_format = a.str("in-format");
    p.out_format = a.str("out-format");
    if (t == "png" || t == "png16") {
        for (const char* k : {"i", "ref", "o"}) {
            if ((std::strcmp(k, "i") == 0 && !encoding) || !a.has(k) || !names_a_pipe(a.str(k))) continue;
            die(std::string(k[0] == 'r' ? "--" : "-") + k + " " + a.str(k) + ": --src-type " + t + " reads and writes a directory of PNG pictures, not a pipe");
        }
        if (a.has("in-format") || a.has("out-format")) die("--in-format / --out-format are for raw and Y4M files: --src-type " + t + " is a directory of PNG pictures");
    }
    if (a.has("ref") && is_dash(a.str("i")) && is_dash(a.str("ref"))) die("-i - together with --ref -: stdin carries one of the two");
    for (const char* k : {"json", "rc-log", "scene-log", "quality-log", "hash-log", "latency-log", "vbv-log"}) {
        if (a.has(k) && is_dash(a.str(k))) {
            die(std::string("--") + k + " -: a log goes to a file of its own" + (a.has("o") && is_dash(a.str("o")) ? " (-o - has the standard output)" : ""));
        }
    }
    if (!encoding) {
        for (const char* k : {"read-ahead", "flush-units", "latency-log"}) {
            if (a.has(k)) die(std::string("--") + k + " is an encoder flag");
        }
        return p;
    }
    p.read_ahead = int_arg(a, "read-ahead", -1, 0, 8);
    if (p.read_ahead > 0 && (t == "png" || t == "png16")) die("--read-ahead reads raw and Y4M sources ahead: --src-type " + t + " is a directory of PNG pictures");
    p.flush_units = int_arg(a, "flush-units", 0, 0, 1) != 0;
    p.latency_log = a.str("latency-log");
    if (a.has("latency-log") && p.latency_log.empty()) die("--latency-log needs a file name");
    return p;
}

// --matrix, --range, --yuv-depth: the colour conversion of RGB sources, refused before anything touches the device
struct ColourArgs {
    bool on = false;       // any of the three flags given
    int matrix = DCVC_MATRIX_BT709, range = DCVC_RANGE_FULL, yuv_depth = 8;
    std::string matrix_name = "bt709", range_name = "full";
    void apply(Geometry& g) const { g.matrix = matrix; g.range = range; g.yuv_depth = yuv_depth; }
};

ColourArgs colour_args(const Args& a)
{
    ColourArgs c;
    c.on = a.has("matrix") || a.has("range") || a.has("yuv-depth");
    if (!c.on) return c;
    c.matrix_name = a.str("matrix", "bt709");
    c.range_name = a.str("range", "full");
    if (c.matrix_name == "bt601") c.matrix = DCVC_MATRIX_BT601;
    else if (c.matrix_name == "bt709") c.matrix = DCVC_MATRIX_BT709;
    else if (c.matrix_name == "bt2020") c.matrix = DCVC_MATRIX_BT2020;
    else die("unknown --matrix " + c.matrix_name + " (bt601, bt709 or bt2020)");
    if (c.range_name == "full") c.range = DCVC_RANGE_FULL;
    else if (c.range_name == "limited") c.range = DCVC_RANGE_LIMITED;
    else die("unknown --range " + c.range_name + " (full or limited)");
    c.yuv_depth = int_arg(a, "yuv-depth", 8, 8, 16);
    if (a.has("yuv-depth") && c.range != DCVC_RANGE_LIMITED) {
        die("--yuv-depth needs --range limited: the depth places the limited-range levels, full range does not depend on it");
    }
    // a Y4M -i or --ref cannot make the type RGB: a header that disagrees with --src-type is refused
    const std::string t = a.str("src-type", "yuv420");
    if (!is_rgb_name(t)) {
        die("--matrix, --range and --yuv-depth are for --src-type rgb24 and png: " + t + " pictures are not converted");
    }
    return c;
}

RateArgs rate_args(const Args& a, int batch)
{
    RateArgs r;
    if (!a.has("target-bpp")) {
        for (const char* k : {"qp-min", "qp-max", "rc-horizon", "rc-intra-bonus", "rc-log", "rc-mode"}) {
            if (a.has("target-psnr") && (std::strcmp(k, "qp-min") == 0 || std::strcmp(k, "qp-max") == 0)) continue;      // quality_args
            if (a.has(k)) die(std::string("--") + k + " needs --target-bpp");
        }
        return r;
    }
    r.on = true;
    const std::string s = a.str("target-bpp");
    char* end = nullptr;
    r.target_bpp = strtod(s.c_str(), &end);
    if (s.empty() || *end != '\0' || !std::isfinite(r.target_bpp) || !(r.target_bpp > 0)) {
        die("--target-bpp must be a positive number of bits per pixel, got " + s);
    }
    if (batch > 1) die("--target-bpp cannot be combined with --batch above 1: a batch has one q_index");
    if (a.has("qp-p")) die("--target-bpp cannot be combined with --qp-p: the controller chooses the q_index of the P units");
    r.qp_min = int_arg(a, "qp-min", 0, 0, 63);
    r.qp_max = int_arg(a, "qp-max", 63, 0, 63);
    if (r.qp_min > r.qp_max) die("--qp-min " + std::to_string(r.qp_min) + " is above --qp-max " + std::to_string(r.qp_max));
    r.horizon = int_arg(a, "rc-horizon", 8, 1, 1 << 20);
    r.intra_bonus = int_arg(a, "rc-intra-bonus", 0, -63, 63);
    r.log = a.str("rc-log");
    const std::string mode = a.str("rc-mode", "feedback");
    if (mode != "feedback" && mode != "probe") die("--rc-mode must be feedback or probe, got " + mode);
    r.probe = mode == "probe";
    return r;
}

// --vbv-maxrate / --vbv-bufsize with --vbv-init and --vbv-log, refused before a model is loaded
struct VbvArgs {
    bool on = false;
    double maxrate = 0, bufsize = 0, init = 0.9;
    std::string log;
};

VbvArgs vbv_args(const Args& a, int batch, bool encoding)
{
    VbvArgs v;
    if (!encoding) {
        for (const char* k : {"vbv-maxrate", "vbv-bufsize", "vbv-init", "vbv-log"}) {
            if (a.has(k)) die(std::string("--") + k + " is an encoder flag");
        }
        return v;
    }
    if (a.has("vbv-maxrate") != a.has("vbv-bufsize")) {
        die(a.has("vbv-maxrate") ? "--vbv-maxrate needs --vbv-bufsize: the rate and the buffer size make the model together"
                                 : "--vbv-bufsize needs --vbv-maxrate: the rate and the buffer size make the model together");
    }
    if (!a.has("vbv-maxrate")) {
        for (const char* k : {"vbv-init", "vbv-log"}) {
            if (a.has(k)) die(std::string("--") + k + " needs --vbv-maxrate and --vbv-bufsize");
        }
        return v;
    }
    v.on = true;
    auto number = [&](const char* k, double def) {
        if (!a.has(k)) return def;
        const std::string s = a.str(k);
        char* end = nullptr;
        const double d = strtod(s.c_str(), &end);
        if (s.empty() || *end != '\0') die(std::string("--") + k + " must be a number, got " + s);
        return d;
    };
    v.maxrate = number("vbv-maxrate", 0);
    v.bufsize = number("vbv-bufsize", 0);
    v.init = number("vbv-init", 0.9);
    // what dcvc_rc_vbv_create refuses of the three values, in its words; the picture size comes later
    dcvc_rc_vbv* probe = dcvc_rc_vbv_create(v.maxrate, v.bufsize, v.init, 1);
    if (!probe) {
        die(std::string("--vbv-maxrate ") + a.str("vbv-maxrate") + " --vbv-bufsize " + a.str("vbv-bufsize") + " --vbv-init " + a.str("vbv-init", "0.9") +
            ": " + dcvc_last_error());
    }
    dcvc_rc_vbv_destroy(probe);
    if (batch > 1) die("--vbv-maxrate cannot be combined with --batch above 1: a batch has one q_index");
    if (a.has("target-psnr")) die("--vbv-maxrate cannot be combined with --target-psnr: coding to a quality under a cap is not built");
    v.log = a.str("vbv-log");
    if (a.has("vbv-log") && v.log.empty()) die("--vbv-log needs a file name");
    return v;
}

// one coded unit in --vbv-log
struct VbvUnit {
    bool intra = false, violated = false;
    int first_picture = 0, pictures = 0, qp_mode = -1, qp = 0, probes = 0, recodes = 0;
    long long predicted_bytes = -1, bytes = 0, underflow_bits = 0;      // -1: no prediction; bytes: what the unit added to the file
    double fullness_before = 0, fullness_after = 0;
};

// --target-psnr with --qp-min / --qp-max, and --quality-log, refused before anything touches the device
struct QualityArgs {
    bool target_on = false;
    double target = 0;
    int qp_min = 0, qp_max = 63;
    std::string log;
    bool on() const { return target_on || !log.empty(); }
};

QualityArgs quality_args(const Args& a, int batch)
{
    QualityArgs q;
    q.log = a.str("quality-log");
    if (a.has("quality-log") && q.log.empty()) die("--quality-log needs a file name");
    if (!a.has("target-psnr")) return q;
    q.target_on = true;
    const std::string s = a.str("target-psnr");
    char* end = nullptr;
    q.target = strtod(s.c_str(), &end);
    if (s.empty() || *end != '\0' || !std::isfinite(q.target) || !(q.target > 0)) {
        die("--target-psnr must be a positive number of dB, got " + s);
    }
    if (a.has("target-bpp")) die("--target-psnr cannot be combined with --target-bpp: a unit is coded to a quality or to a rate");
    if (a.has("qp-p")) die("--target-psnr cannot be combined with --qp-p: the search chooses the q_index of the P units");
    if (batch > 1) die("--target-psnr cannot be combined with --batch above 1: a batch has one q_index");
    q.qp_min = int_arg(a, "qp-min", 0, 0, 63);
    q.qp_max = int_arg(a, "qp-max", 63, 0, 63);
    if (q.qp_min > q.qp_max) die("--qp-min " + std::to_string(q.qp_min) + " is above --qp-max " + std::to_string(q.qp_max));
    return q;
}

// --scene-cut and its companions; what the flags alone decide is refused before a model is loaded
struct SceneArgs {
    bool on = false;
    double threshold = 0;
    int min_gap = 8;
    std::string log;
};

SceneArgs scene_args(const Args& a, int batch)
{
    SceneArgs sc;
    if (!a.has("scene-cut")) {
        for (const char* k : {"scene-min-gap", "scene-log"}) {
            if (a.has(k)) die(std::string("--") + k + " needs --scene-cut");
        }
        return sc;
    }
    sc.on = true;
    const std::string s = a.str("scene-cut");
    char* end = nullptr;
    sc.threshold = strtod(s.c_str(), &end);
    if (s.empty() || *end != '\0' || !std::isfinite(sc.threshold) || !(sc.threshold > 0) || sc.threshold > 100) {
        die("--scene-cut must be a threshold in (0, 100] (percent of full range; 5 is a reasonable start), got " + s);
    }
    sc.min_gap = int_arg(a, "scene-min-gap", 8, 1, 1 << 30);
    if (batch > 1) die("--scene-cut cannot be combined with --batch above 1: a batch holds I pictures only");
    if (!a.has("inter") || a.num("intra-period", -1) == 1) {
        die("--scene-cut is for runs with P pictures: an all-intra run (no --inter, or --intra-period 1) has an I picture at every cut");
    }
    sc.log = a.str("scene-log");
    return sc;
}

// "WxH" of --scale / --out-size: two positive even decimal numbers, nothing else
bool parse_size(const std::string& s, int& w, int& h)
{
    const size_t x = s.find('x');
    if (x == std::string::npos || x == 0 || x + 1 >= s.size()) return false;
    long v[2];
    const std::string part[2] = {s.substr(0, x), s.substr(x + 1)};
    for (int i = 0; i < 2; ++i) {
        if (part[i].size() > 6 || part[i].find_first_not_of("0123456789") != std::string::npos) return false;
        v[i] = strtol(part[i].c_str(), nullptr, 10);
        if (v[i] < 2 || (v[i] & 1)) return false;
    }
    w = static_cast<int>(v[0]); h = static_cast<int>(v[1]);
    return true;
}

// --scale (encode) / --out-size (decode): what the flag alone decides is refused before a model is loaded
struct SizeArg {
    bool on = false;
    int W = 0, H = 0;
};

SizeArg size_arg(const Args& a, const char* key)
{
    SizeArg z;
    if (!a.has(key)) return z;
    const std::string flag = std::string("--") + key;
    const std::string type = a.str("src-type", "yuv420");
    if (is_rgb_name(type)) die(flag + " is for --src-type yuv420: RGB sources are not resampled yet");
    if (type == "yuv422" || type == "yuv444" || type == "nv12" || type == "p010" || wire_of(type) >= 0) {
        die(flag + " is for --src-type yuv420: " + type + " sources are not resampled yet");
    }
    if (!parse_size(a.str(key), z.W, z.H)) die(flag + " must be WxH with both sides positive and even, got " + a.str(key));
    z.on = true;
    return z;
}

// each side's ratio in [1/8, 8] (dcvc_resample_ntaps is host code: no device is touched)
void check_ratio(const char* flag, int from_w, int from_h, int to_w, int to_h)
{
    if (dcvc_resample_ntaps(from_w, to_w) < 0 || dcvc_resample_ntaps(from_h, to_h) < 0) {
        die(std::string(flag) + ": each side's ratio must lie in [1/8, 8], got " + std::to_string(from_w) + "x" + std::to_string(from_h) +
            " -> " + std::to_string(to_w) + "x" + std::to_string(to_h));
    }
}

// the YUV420 planes of one picture at another size on the device: Y in one call, U and V in one call
struct Resampler {
    void* plan_y = nullptr;
    void* plan_c = nullptr;
    void* ws = nullptr;
    long long ws_bytes = 0;
    int from_h = 0, from_w = 0, to_h = 0, to_w = 0, bit_depth = 8;
    void create(int fh, int fw, int th, int tw, int depth)
    {
        from_h = fh; from_w = fw; to_h = th; to_w = tw; bit_depth = depth;
        abi_ok(dcvc_resample_plan_create(fh, fw, th, tw, &plan_y), "resample plan");
        abi_ok(dcvc_resample_plan_create(fh / 2, fw / 2, th / 2, tw / 2, &plan_c), "resample plan");
        ws_bytes = std::max(dcvc_resample_workspace_bytes(plan_y, 1), dcvc_resample_workspace_bytes(plan_c, 2));
        hip_ok(hipMalloc(&ws, static_cast<size_t>(ws_bytes)), "hipMalloc");
    }
    // src / dst: the planes Y [h][w], U, V [h/2][w/2] back to back, u8 or u16 by the bit depth
    void run(const uint8_t* src, uint8_t* dst, hipStream_t st) const
    {
        const int es = bit_depth > 8 ? 2 : 1, dt = bit_depth > 8 ? DCVC_SAMPLE_U16 : DCVC_SAMPLE_U8, max_val = (1 << bit_depth) - 1;
        const long long fy = static_cast<long long>(from_h) * from_w, ty = static_cast<long long>(to_h) * to_w;
        abi_ok(dcvc_resample_planes(plan_y, src, dt, from_w, fy, dst, dt, to_w, ty, 1, max_val, ws, ws_bytes, st), "resample (Y)");
        abi_ok(dcvc_resample_planes(plan_c, src + fy * es, dt, from_w / 2, fy / 4, dst + ty * es, dt, to_w / 2, ty / 4, 2, max_val, ws,
                                    ws_bytes, st), "resample (U, V)");
    }
    void destroy()
    {
        if (ws) hip_ok(hipFree(ws), "hipFree");
        abi_ok(dcvc_resample_plan_free(plan_y), "resample plan");
        abi_ok(dcvc_resample_plan_free(plan_c), "resample plan");
        *this = Resampler{};
    }
};

// ------------------------------------------------------------------------------------ film grain
// encode --denoise S[:T] --grain-log FILE measures what the filter removes (dcvc_grain_stats) and fits grain records
// (dcvc_grain_fit); decode --film-grain FILE / --grain-strength Y[:C[:SIZE]] puts grain of those records onto the output pictures
// (dcvc_grain_template, dcvc_grain_apply). The defaults below are untuned first guesses.
constexpr int kGrainSize = 12, kGrainGain = 100, kGrainFlat = 4, kGrainMinCount = 256;

struct GrainRecord {
    long long first = 0, pictures = 0;     // output pictures first .. first + pictures - 1 (the last record: and all that follow)
    uint32_t seed = 1;
    int size = kGrainSize;
    uint8_t lut[27] = {};                  // [3][9]: Y, U, V
    uint64_t words[48] = {};               // [3][16]: the window's summed dcvc_grain_stats words
};

struct GrainFile {
    int bit_depth = 0, width = 0, height = 0, spatial = 0, temporal = 0;      // bit_depth 0: --grain-strength, which fits any run
    std::string chroma;
    std::vector<GrainRecord> records;
};

// a decimal integer in 0..max, digits only
bool parse_uint(const std::string& s, unsigned long long max, unsigned long long& v)
{
    if (s.empty() || s.size() > 20 || s.find_first_not_of("0123456789") != std::string::npos || (s.size() > 1 && s[0] == '0')) return false;
    errno = 0;
    v = strtoull(s.c_str(), nullptr, 10);
    return errno == 0 && v <= max;
}

// the JSON a grain file needs: objects, arrays, strings without escapes and non-negative integers
struct Json {
    enum Kind { Number, String, Array, Object, Literal } kind = Number;      // Literal: null, true or false (a crop log)
    std::string text;                      // a number's digits, a string's characters, a literal's name
    std::vector<std::string> keys;         // an object's keys, beside items
    std::vector<Json> items;
    const Json* get(const std::string& k) const
    {
        for (size_t i = 0; i < keys.size(); ++i) {
            if (keys[i] == k) return &items[i];
        }
        return nullptr;
    }
};

struct JsonReader {
    const std::string& s;
    std::function<void(const std::string&)> bad;
    size_t at = 0;
    void space()
    {
        while (at < s.size() && (s[at] == ' ' || s[at] == '\n' || s[at] == '\t' || s[at] == '\r')) ++at;
    }
    bool take(char c)
    {
        space();
        if (at < s.size() && s[at] == c) { ++at; return true; }
        return false;
    }
    std::string string()
    {
        if (!take('"')) bad("a string is expected at byte " + std::to_string(at));
        const size_t end = s.find('"', at);
        if (end == std::string::npos) bad("a string does not end");
        const std::string t = s.substr(at, end - at);
        if (t.find('\\') != std::string::npos) bad("escapes in strings are not read");
        at = end + 1;
        return t;
    }
    Json value(int depth)
    {
        if (depth > 6) bad("nested too deep");
        Json v;
        space();
        if (at >= s.size()) bad("the text ends inside a value");
        const char c = s[at];
        if (c == '{' || c == '[') {
            const char close = c == '{' ? '}' : ']';
            v.kind = c == '{' ? Json::Object : Json::Array;
            ++at;
            if (take(close)) return v;
            do {
                if (v.kind == Json::Object) {
                    v.keys.push_back(string());
                    if (!take(':')) bad("no ':' behind the key " + v.keys.back());
                }
                v.items.push_back(value(depth + 1));
            } while (take(','));
            if (!take(close)) bad(std::string("no '") + close + "' at byte " + std::to_string(at));
        } else if (c == '"') {
            v.kind = Json::String;
            v.text = string();
        } else if (c >= 'a' && c <= 'z') {
            const size_t end = s.find_first_not_of("abcdefghijklmnopqrstuvwxyz", at);
            v.kind = Json::Literal;
            v.text = s.substr(at, end == std::string::npos ? end : end - at);
            if (v.text != "null" && v.text != "true" && v.text != "false") bad("the word " + v.text + " at byte " + std::to_string(at));
            at += v.text.size();
        } else {
            const size_t end = s.find_first_not_of("0123456789", at);
            v.text = s.substr(at, end == std::string::npos ? end : end - at);
            if (v.text.empty()) bad("a non-negative integer, a string, an array or an object is expected at byte " + std::to_string(at));
            at += v.text.size();
        }
        return v;
    }
};

const char* chroma_name(const Geometry& g)
{
    return g.pix_fmt == DCVC_PIX_YUV422P ? "yuv422" : g.pix_fmt == DCVC_PIX_YUV444P ? "yuv444" : "yuv420";
}

// the structure of a grain file, strictly; whether it fits the run is decode's business
GrainFile read_grain_file(const std::string& path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) die("--film-grain: cannot open " + path);
    const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::function<void(const std::string&)> bad = [&](const std::string& why) { die("--film-grain: " + path + " is no grain file: " + why); };
    JsonReader rd{text, bad};
    const Json top = rd.value(0);
    rd.space();
    if (rd.at != text.size()) bad("text behind the value");
    if (top.kind != Json::Object) bad("no object");
    auto num = [&](const Json& o, const std::string& key, unsigned long long lo, unsigned long long hi) {
        const Json* v = o.get(key);
        unsigned long long n = 0;
        if (!v || v->kind != Json::Number || !parse_uint(v->text, hi, n) || n < lo) {
            bad("\"" + key + "\" must be an integer in " + std::to_string(lo) + ".." + std::to_string(hi));
        }
        return n;
    };
    auto list = [&](const Json& o, const std::string& key, size_t count) -> const Json& {
        const Json* v = o.get(key);
        if (!v || v->kind != Json::Array || v->items.size() != count) bad("\"" + key + "\" must be a list of " + std::to_string(count));
        return *v;
    };
    auto elem = [&](const Json& l, size_t i, const std::string& key, unsigned long long hi) {
        unsigned long long n = 0;
        if (l.items[i].kind != Json::Number || !parse_uint(l.items[i].text, hi, n)) bad("\"" + key + "\" holds integers in 0.." + std::to_string(hi));
        return n;
    };
    GrainFile g;
    if (num(top, "version", 0, 1000000) != 1) bad("version " + top.get("version")->text + " (this tool reads version 1)");
    g.bit_depth = static_cast<int>(num(top, "bit_depth", 8, 16));
    const Json* cf = top.get("chroma_format");
    if (!cf || cf->kind != Json::String || (cf->text != "yuv420" && cf->text != "yuv422" && cf->text != "yuv444")) {
        bad("\"chroma_format\" must be yuv420, yuv422 or yuv444");
    }
    g.chroma = cf->text;
    g.width = static_cast<int>(num(top, "width", 2, kMaxPictureSide));
    g.height = static_cast<int>(num(top, "height", 2, kMaxPictureSide));
    const Json& dn = list(top, "denoise", 2);
    g.spatial = static_cast<int>(elem(dn, 0, "denoise", 64));
    g.temporal = static_cast<int>(elem(dn, 1, "denoise", 64));
    const Json* recs = top.get("records");
    if (!recs || recs->kind != Json::Array || recs->items.empty()) bad("\"records\" must be a list of at least one record");
    long long next = 0;
    for (const Json& r : recs->items) {
        if (r.kind != Json::Object) bad("a record is no object");
        GrainRecord rec;
        rec.first = static_cast<long long>(num(r, "first", 0, 1ull << 40));
        if (rec.first != next) bad("record " + std::to_string(g.records.size()) + " must start at picture " + std::to_string(next));
        rec.pictures = static_cast<long long>(num(r, "pictures", 1, 1ull << 40));
        next = rec.first + rec.pictures;
        rec.seed = static_cast<uint32_t>(num(r, "seed", 0, 0xFFFFFFFFull));
        rec.size = static_cast<int>(num(r, "size", 0, 37));
        const char* names[3] = {"y", "u", "v"};
        for (int p = 0; p < 3; ++p) {
            const Json& t = list(r, names[p], 9);
            for (size_t k = 0; k < 9; ++k) rec.lut[9 * p + static_cast<int>(k)] = static_cast<uint8_t>(elem(t, k, names[p], 255));
        }
        const Json& w = list(r, "words", 3);
        for (size_t p = 0; p < 3; ++p) {
            if (w.items[p].kind != Json::Array || w.items[p].items.size() != 16) bad("\"words\" must hold three lists of 16");
            for (size_t k = 0; k < 16; ++k) rec.words[16 * p + k] = elem(w.items[p], k, "words", (1ull << 63) - 1);
        }
        g.records.push_back(rec);
    }
    return g;
}

std::string grain_file_text(const GrainFile& g)
{
    std::string s = "{\n  \"version\": 1,\n  \"bit_depth\": " + std::to_string(g.bit_depth) + ",\n  \"chroma_format\": \"" + g.chroma +
                    "\",\n  \"width\": " + std::to_string(g.width) + ",\n  \"height\": " + std::to_string(g.height) + ",\n  \"denoise\": [" +
                    std::to_string(g.spatial) + ", " + std::to_string(g.temporal) + "],\n  \"records\": [";
    for (size_t i = 0; i < g.records.size(); ++i) {
        const GrainRecord& r = g.records[i];
        s += std::string(i ? "," : "") + "\n    {\"first\": " + std::to_string(r.first) + ", \"pictures\": " + std::to_string(r.pictures) +
             ", \"seed\": " + std::to_string(r.seed) + ", \"size\": " + std::to_string(r.size);
        const char* names[3] = {"y", "u", "v"};
        for (int p = 0; p < 3; ++p) {
            s += std::string(",\n     \"") + names[p] + "\": [";
            for (int k = 0; k < 9; ++k) s += (k ? ", " : "") + std::to_string(r.lut[9 * p + k]);
            s += "]";
        }
        s += ",\n     \"words\": [";
        for (int p = 0; p < 3; ++p) {
            s += p ? ", [" : "[";
            for (int k = 0; k < 16; ++k) s += (k ? ", " : "") + std::to_string(r.words[16 * p + k]);
            s += "]";
        }
        s += "]}";
    }
    return s + "\n  ]\n}\n";
}

// what the flags alone decide is refused before a model is loaded; --film-grain's file is read there too
struct GrainArgs {
    bool on = false;                       // decode: pictures are grained
    bool from_file = false;
    std::string flag;                      // "--film-grain" or "--grain-strength"
    GrainFile file;
    bool log_on = false;                   // encode: --grain-log
    std::string log;
    int size = kGrainSize, window = 0, gain = kGrainGain, flat = kGrainFlat;
    uint32_t seed = 1;
};

GrainArgs grain_args(const Args& a, bool encoding)
{
    GrainArgs g;
    const char* enc_flags[] = {"grain-log", "grain-size", "grain-window", "grain-gain", "grain-flat", "grain-seed"};
    if (encoding) {
        for (const char* k : {"film-grain", "grain-strength"}) {
            if (a.has(k)) die(std::string("--") + k + " is a decoder flag: encode measures the grain with --denoise S[:T] --grain-log FILE");
        }
        if (!a.has("grain-log")) {
            for (const char* k : enc_flags) {
                if (a.has(k)) die(std::string("--") + k + " needs --grain-log");
            }
            return g;
        }
        if (!a.has("denoise")) die("--grain-log needs --denoise: it measures what the filter removes");
        g.log = a.str("grain-log");
        if (g.log.empty() || is_dash(g.log)) die("--grain-log needs a file name (not -: stdout is for the stream)");
        auto opt = [&](const char* k, unsigned long long lo, unsigned long long hi, unsigned long long def) {
            unsigned long long v = def;
            if (a.has(k) && (!parse_uint(a.str(k), hi, v) || v < lo)) {
                die(std::string("--") + k + " must be an integer in " + std::to_string(lo) + ".." + std::to_string(hi) + ", got " + a.str(k));
            }
            return v;
        };
        g.size = static_cast<int>(opt("grain-size", 0, 37, kGrainSize));
        g.window = static_cast<int>(opt("grain-window", 0, 1 << 30, 0));
        g.gain = static_cast<int>(opt("grain-gain", 1, 400, kGrainGain));
        g.flat = static_cast<int>(opt("grain-flat", 0, 255, kGrainFlat));
        g.seed = static_cast<uint32_t>(opt("grain-seed", 0, 0xFFFFFFFFull, 1));
        g.log_on = true;
        return g;
    }
    for (const char* k : enc_flags) {
        if (a.has(k)) die(std::string("--") + k + " is an encoder flag");
    }
    if (a.has("film-grain") && a.has("grain-strength")) die("--film-grain and --grain-strength: exactly one of them may be given");
    if (!a.has("film-grain") && !a.has("grain-strength")) return g;
    g.flag = a.has("film-grain") ? "--film-grain" : "--grain-strength";
    if (!a.has("o") && !a.has("hash-log") && !a.has("verify-hash")) {
        die(g.flag + " changes what -o writes and the hashes cover, nothing else: it needs -o, --hash-log or --verify-hash");
    }
    const std::string type = a.str("src-type", "yuv420");
    if (type != "yuv420" && type != "yuv422" && type != "yuv444") {
        die(g.flag + " is for planar YUV pictures: " + type + " pictures are not grained yet");
    }
    if (a.has("film-grain")) {
        if (a.str("film-grain").empty()) die("--film-grain needs a file name");
        g.file = read_grain_file(a.str("film-grain"));
        g.from_file = true;
    } else {
        // Y[:C[:SIZE]]: constant tables in sixteenths of an 8-bit code value, C = Y and SIZE = 12 when left out
        const std::string s = a.str("grain-strength");
        std::vector<std::string> part;
        for (size_t at = 0; at <= s.size();) {
            const size_t colon = std::min(s.find(':', at), s.size());
            part.push_back(s.substr(at, colon - at));
            at = colon + 1;
        }
        unsigned long long v[3] = {0, 0, static_cast<unsigned long long>(kGrainSize)};
        bool ok = part.size() >= 1 && part.size() <= 3;
        for (size_t i = 0; ok && i < part.size(); ++i) ok = parse_uint(part[i], i == 2 ? 37 : 255, v[i]);
        if (!ok) die("--grain-strength must be Y, Y:C or Y:C:SIZE with Y and C in 0..255 and SIZE in 0..37, got " + s);
        if (part.size() == 1) v[1] = v[0];
        GrainRecord r;
        r.pictures = 1;
        r.size = static_cast<int>(v[2]);
        for (int k = 0; k < 27; ++k) r.lut[k] = static_cast<uint8_t>(k < 9 ? v[0] : v[1]);
        g.file.records.push_back(r);
    }
    g.on = true;
    return g;
}

// the file against the run's pictures, once their type and depth are settled (a Y4M --ref may supply them)
void grain_check_run(const GrainArgs& ga, const char* type, int depth)
{
    const std::string t = type;
    if (t != "yuv420" && t != "yuv422" && t != "yuv444") die(ga.flag + " is for planar YUV pictures: " + t + " pictures are not grained yet");
    if (!ga.from_file) return;
    if (ga.file.bit_depth != depth || ga.file.chroma != t) {
        die("--film-grain: the file describes " + ga.file.chroma + " pictures of " + std::to_string(ga.file.bit_depth) + " bits, this run's are " + t +
            " of " + std::to_string(depth) + " bits");
    }
}

// decode: the output picture in `rec` (planes Y, U, V back to back) -> the grained picture in a buffer of the stage's own; rec
// stays as it is (the metrics read it). Templates are made on the host and uploaded when a record starts.
struct GrainSynth {
    GrainArgs arg;
    uint8_t* out = nullptr;
    int16_t* d_tpl = nullptr;
    int16_t* h_tpl = nullptr;              // pinned
    int current = -1;
    long long pic = 0;                     // the output picture's index in output order
    void create(const Geometry& og, const GrainArgs& ga)
    {
        arg = ga;
        if (out) hip_ok(hipFree(out), "hipFree");
        hip_ok(hipMalloc(&out, og.frame_bytes()), "hipMalloc");
        if (d_tpl) return;
        hip_ok(hipMalloc(&d_tpl, 3 * 4096 * sizeof(int16_t)), "hipMalloc");
        hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_tpl), 3 * 4096 * sizeof(int16_t), hipHostMallocDefault), "hipHostMalloc");
    }
    const uint8_t* run(const Geometry& og, const uint8_t* rec, hipStream_t st)
    {
        const std::vector<GrainRecord>& rs = arg.file.records;
        int r = std::max(current, 0);
        while (r + 1 < static_cast<int>(rs.size()) && pic >= rs[static_cast<size_t>(r) + 1].first) ++r;      // past the last record: it stays
        if (r != current) {
            hip_ok(hipStreamSynchronize(st), "sync");      // the previous record's templates may still be on their way
            for (int p = 0; p < 3; ++p) abi_ok(dcvc_grain_template(rs[static_cast<size_t>(r)].seed, p, rs[static_cast<size_t>(r)].size, h_tpl + 4096 * p), "grain template");
            hip_ok(hipMemcpyAsync(d_tpl, h_tpl, 3 * 4096 * sizeof(int16_t), hipMemcpyHostToDevice, st), "H2D");
            current = r;
        }
        const GrainRecord& g = rs[static_cast<size_t>(r)];
        const int es = og.hbd() ? 2 : 1, dt = og.hbd() ? DCVC_SAMPLE_U16 : DCVC_SAMPLE_U8;
        const long long ny = static_cast<long long>(og.H) * og.W, nc = static_cast<long long>(og.Hc()) * og.Wc();
        const int sx = og.Wc() != og.W ? 1 : 0, sy = og.Hc() != og.H ? 1 : 0;
        const uint32_t idx = static_cast<uint32_t>(pic);
        abi_ok(dcvc_grain_apply(rec, og.W, ny, rec, og.W, og.H, og.W, out, og.W, ny, dt, og.bit_depth, og.H, og.W, 1, 0, 0, 0, d_tpl, d_tpl + 4096,
                                d_tpl + 8192, g.lut, g.seed, idx, st), "grain (Y)");
        abi_ok(dcvc_grain_apply(rec + ny * es, og.Wc(), nc, rec, og.W, og.H, og.W, out + ny * es, og.Wc(), nc, dt, og.bit_depth, og.Hc(), og.Wc(), 2,
                                1, sx, sy, d_tpl, d_tpl + 4096, d_tpl + 8192, g.lut, g.seed, idx, st), "grain (U, V)");
        ++pic;
        return out;
    }
    void destroy()
    {
        if (out) hip_ok(hipFree(out), "hipFree");
        if (d_tpl) hip_ok(hipFree(d_tpl), "hipFree");
        if (h_tpl) hip_ok(hipHostFree(h_tpl), "hipHostFree");
        *this = GrainSynth{};
    }
};

// encode: what the denoiser took out of every source picture, summed on the device and, every 8 pictures, on the host (8 calls
// of less than 2^60 a word stay below 2^63); a record is fitted at the end of every window of source pictures
struct GrainMeter {
    GrainArgs arg;
    GrainFile file;
    uint64_t* d_words = nullptr;
    uint64_t* h_words = nullptr;           // pinned
    uint64_t sum[48] = {};
    int on_device = 0;                     // pictures summed in d_words
    long long in_window = 0, first = 0;
    void create(const Geometry& g, const GrainArgs& ga, int spatial, int temporal)
    {
        arg = ga;
        file.bit_depth = g.bit_depth; file.chroma = chroma_name(g); file.width = g.W; file.height = g.H;
        file.spatial = spatial; file.temporal = temporal;
        hip_ok(hipMalloc(&d_words, 48 * sizeof(uint64_t)), "hipMalloc");
        hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_words), 48 * sizeof(uint64_t), hipHostMallocDefault), "hipHostMalloc");
    }
    // src: a source picture at the coded size, den: the filter's output for it (planes Y, U, V back to back)
    void measure(const Geometry& g, const uint8_t* src, const uint8_t* den, hipStream_t st)
    {
        const int es = g.hbd() ? 2 : 1, dt = g.hbd() ? DCVC_SAMPLE_U16 : DCVC_SAMPLE_U8;
        const long long ny = static_cast<long long>(g.H) * g.W, nc = static_cast<long long>(g.Hc()) * g.Wc();
        const int sx = g.Wc() != g.W ? 1 : 0, sy = g.Hc() != g.H ? 1 : 0, acc = on_device > 0 ? 1 : 0;
        abi_ok(dcvc_grain_stats(src, g.W, ny, den, g.W, ny, den, g.W, g.H, g.W, dt, g.bit_depth, g.H, g.W, 1, 0, 0, arg.flat, acc, d_words, st),
               "grain stats (Y)");
        abi_ok(dcvc_grain_stats(src + ny * es, g.Wc(), nc, den + ny * es, g.Wc(), nc, den, g.W, g.H, g.W, dt, g.bit_depth, g.Hc(), g.Wc(), 2, sx, sy,
                                arg.flat, acc, d_words + 16, st), "grain stats (U, V)");
        ++in_window;
        if (++on_device == 8) flush(st);
        if (arg.window > 0 && in_window == arg.window) close(st);
    }
    void flush(hipStream_t st)
    {
        if (on_device == 0) return;
        hip_ok(hipMemcpyAsync(h_words, d_words, 48 * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H");
        hip_ok(hipStreamSynchronize(st), "sync");
        for (int i = 0; i < 48; ++i) {
            sum[i] += h_words[i];
            if (sum[i] >> 63) die("--grain-log: a window's sums pass 2^63; use a shorter --grain-window");
        }
        on_device = 0;
    }
    void close(hipStream_t st)
    {
        flush(st);
        if (in_window == 0) return;
        GrainRecord r;
        r.first = first; r.pictures = in_window;
        r.seed = arg.seed + static_cast<uint32_t>(file.records.size());
        r.size = arg.size;
        std::memcpy(r.words, sum, sizeof(sum));
        abi_ok(dcvc_grain_fit(sum, file.bit_depth, arg.gain, kGrainMinCount, r.lut), "grain fit");
        file.records.push_back(r);
        first += in_window;
        in_window = 0;
        std::memset(sum, 0, sizeof(sum));
    }
    void finish(hipStream_t st)
    {
        close(st);
        const std::string text = grain_file_text(file);
        FILE* lf = fopen(arg.log.c_str(), "wb");
        if (!lf || fwrite(text.data(), 1, text.size(), lf) != text.size() || fclose(lf) != 0) die("cannot write " + arg.log);
        fprintf(g_msg, "grain: %zu record%s over %lld pictures (size %d, gain %d%%, flat %d, window %d) -> %s\n", file.records.size(),
                file.records.size() == 1 ? "" : "s", first, arg.size, arg.gain, arg.flat, arg.window, arg.log.c_str());
        hip_ok(hipFree(d_words), "hipFree");
        hip_ok(hipHostFree(h_words), "hipHostFree");
        d_words = h_words = nullptr;
    }
};

// --denoise S[:T] / --denoise-out FILE (encode): what the flags alone decide is refused before a model is loaded
struct DenoiseArgs {
    bool on = false;
    int spatial = 0, temporal = 0;
    std::string out;               // --denoise-out: the filtered clip as coded, raw
    bool mc = false;               // --denoise-mc R[:LAMBDA]
    int mc_range = 0, mc_lambda = 4;
    std::string mv_log;            // --mv-log: what the search found, JSON
};

// "R" or "R:LAMBDA": decimal integers in 0..15 and 0..255, nothing else
bool parse_mc(const std::string& s, int& range, int& lambda)
{
    const size_t colon = s.find(':');
    unsigned long long r = 0, l = 4;
    if (!parse_uint(s.substr(0, colon), 15, r)) return false;
    if (colon != std::string::npos && !parse_uint(s.substr(colon + 1), 255, l)) return false;
    range = static_cast<int>(r); lambda = static_cast<int>(l);
    return true;
}

// "S" or "S:T": decimal integers in 0..64, nothing else
bool parse_strengths(const std::string& s, int& spatial, int& temporal)
{
    const size_t colon = s.find(':');
    const std::string part[2] = {s.substr(0, colon), colon == std::string::npos ? s.substr(0, colon) : s.substr(colon + 1)};
    int v[2];
    for (int i = 0; i < 2; ++i) {
        if (part[i].empty() || part[i].size() > 2 || part[i].find_first_not_of("0123456789") != std::string::npos) return false;
        v[i] = atoi(part[i].c_str());
        if (v[i] > 64) return false;
    }
    spatial = v[0]; temporal = v[1];
    return true;
}

DenoiseArgs denoise_args(const Args& a, bool encoding)
{
    DenoiseArgs d;
    if (!encoding) {
        for (const char* k : {"denoise", "denoise-out", "denoise-mc", "mv-log"}) {
            if (a.has(k)) die(std::string("--") + k + " is an encoder flag");
        }
        return d;
    }
    if (!a.has("denoise")) {
        for (const char* k : {"denoise-out", "denoise-mc", "mv-log"}) {
            if (a.has(k)) die(std::string("--") + k + " needs --denoise");
        }
        return d;
    }
    if (a.has("mv-log") && !a.has("denoise-mc")) die("--mv-log needs --denoise-mc");
    if (a.has("denoise-mc")) {
        if (!parse_mc(a.str("denoise-mc"), d.mc_range, d.mc_lambda)) {
            die("--denoise-mc must be R or R:LAMBDA with integers in 0..15 and 0..255, got " + a.str("denoise-mc"));
        }
        d.mc = true;
        d.mv_log = a.str("mv-log");
        if (a.has("mv-log") && (d.mv_log.empty() || is_dash(d.mv_log))) die("--mv-log needs a file name (not -: stdout is for the stream)");
    }
    if (!parse_strengths(a.str("denoise"), d.spatial, d.temporal)) {
        die("--denoise must be S or S:T with integers in 0..64, got " + a.str("denoise"));
    }
    const std::string type = a.str("src-type", "yuv420");
    if (is_rgb_name(type)) die("--denoise is for planar YUV sources: RGB sources are not filtered yet");
    if (type == "nv12" || type == "p010" || type == "nv21") {
        die("--denoise is for planar YUV sources: " + type + " sources are not filtered yet");
    }
    d.out = a.str("denoise-out");
    if (a.has("denoise-out") && (d.out.empty() || is_dash(d.out))) die("--denoise-out needs a file name (not -: stdout is for the stream)");
    d.on = true;
    return d;
}

// --denoise: the planes of a picture at the coded size through dcvc_denoise_planes, Y in one call, U and V in one call. The
// state is the previous output picture, on the device in two buffers used in turn.
struct Denoiser {
    DenoiseArgs arg;
    uint8_t* hist[2] = {nullptr, nullptr};
    uint8_t* h_out = nullptr;      // pinned: --denoise-out's picture
    FILE* file = nullptr;
    int turn = 0;
    long long pictures = 0;
    GrainMeter* meter = nullptr;   // --grain-log: every source picture and the filter's output for it are measured
    // --denoise-mc: the previous output picture motion-compensated, the vectors, their SADs, the count of moved blocks and the
    // search's workspace, all on the device; h_mv (pinned: vectors, then SADs) only with --mv-log
    uint8_t* comp = nullptr;
    int16_t* d_mv = nullptr;
    uint32_t* d_sad = nullptr;
    uint32_t* d_moved = nullptr;
    void* d_ws = nullptr;
    long long ws_bytes = 0;
    uint8_t* h_mv = nullptr;
    int bh = 0, bw = 0;
    long long searched = 0;        // pictures that went through the search
    std::string mv_records;
    void create(const Geometry& g, const DenoiseArgs& d)
    {
        arg = d;
        for (uint8_t*& p : hist) hip_ok(hipMalloc(&p, g.frame_bytes()), "hipMalloc");
        if (arg.mc && arg.temporal > 0) {
            bh = (g.H + 15) / 16; bw = (g.W + 15) / 16;
            ws_bytes = dcvc_motion_search_workspace_bytes(g.H, g.W);
            if (ws_bytes <= 0) die("--denoise-mc: the coded size is outside the search's limits");
            hip_ok(hipMalloc(&comp, g.frame_bytes()), "hipMalloc");
            hip_ok(hipMalloc(&d_mv, static_cast<size_t>(bh) * bw * 2 * sizeof(int16_t)), "hipMalloc");
            hip_ok(hipMalloc(&d_sad, static_cast<size_t>(bh) * bw * sizeof(uint32_t)), "hipMalloc");
            hip_ok(hipMalloc(&d_moved, sizeof(uint32_t)), "hipMalloc");
            hip_ok(hipMemset(d_moved, 0, sizeof(uint32_t)), "hipMemset");
            hip_ok(hipMalloc(&d_ws, static_cast<size_t>(ws_bytes)), "hipMalloc");
            if (!arg.mv_log.empty()) {
                hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_mv), static_cast<size_t>(bh) * bw * 8, hipHostMallocDefault), "hipHostMalloc");
            }
        }
        if (!arg.out.empty()) {
            hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_out), g.frame_bytes(), hipHostMallocDefault), "hipHostMalloc");
            file = fopen(arg.out.c_str(), "wb");
            if (!file) die("cannot write " + arg.out);
        }
    }
    // the picture in `src` (planes Y, U, V back to back, u8 or u16 by the bit depth) -> the filtered picture, which stays valid
    // until the call after the next one
    uint8_t* run(const Geometry& g, const uint8_t* src, hipStream_t st)
    {
        const int es = g.hbd() ? 2 : 1, dt = g.hbd() ? DCVC_SAMPLE_U16 : DCVC_SAMPLE_U8;
        const long long ny = static_cast<long long>(g.H) * g.W, nc = static_cast<long long>(g.Hc()) * g.Wc();
        const uint8_t* prev = pictures > 0 ? hist[turn ^ 1] : nullptr;
        uint8_t* dst = hist[turn];
        if (prev && comp) {
            const int sx = g.Wc() != g.W ? 1 : 0, sy = g.Hc() != g.H ? 1 : 0;
            abi_ok(dcvc_motion_search(src, g.W, prev, g.W, dt, g.bit_depth, g.H, g.W, arg.mc_range, arg.mc_lambda, d_mv, bh, bw, d_sad, d_moved,
                                      d_ws, ws_bytes, st), "motion search");
            abi_ok(dcvc_motion_compensate_planes(prev, g.W, ny, comp, g.W, ny, dt, g.H, g.W, 1, 0, 0, d_mv, bh, bw, st), "motion compensate (Y)");
            abi_ok(dcvc_motion_compensate_planes(prev + ny * es, g.Wc(), nc, comp + ny * es, g.Wc(), nc, dt, g.Hc(), g.Wc(), 2, sx, sy, d_mv,
                                                 bh, bw, st), "motion compensate (U, V)");
            if (h_mv) log_vectors(st);
            ++searched;
            prev = comp;
        }
        abi_ok(dcvc_denoise_planes(src, g.W, ny, prev, g.W, ny, dst, g.W, ny, dt, g.bit_depth, g.H, g.W, 1, arg.spatial, arg.temporal, st),
               "denoise (Y)");
        abi_ok(dcvc_denoise_planes(src + ny * es, g.Wc(), nc, prev ? prev + ny * es : nullptr, g.Wc(), nc, dst + ny * es, g.Wc(), nc, dt,
                                   g.bit_depth, g.Hc(), g.Wc(), 2, arg.spatial, arg.temporal, st), "denoise (U, V)");
        if (meter) meter->measure(g, src, dst, st);
        if (file) {
            hip_ok(hipMemcpyAsync(h_out, dst, g.frame_bytes(), hipMemcpyDeviceToHost, st), "D2H");
            hip_ok(hipStreamSynchronize(st), "sync");
            if (fwrite(h_out, 1, g.frame_bytes(), file) != g.frame_bytes()) die("cannot write " + arg.out);
        }
        turn ^= 1;
        ++pictures;
        return dst;
    }
    // --mv-log: the vectors and SADs of the picture just searched -> one record
    void log_vectors(hipStream_t st)
    {
        const size_t nb = static_cast<size_t>(bh) * bw;
        hip_ok(hipMemcpyAsync(h_mv, d_mv, nb * 4, hipMemcpyDeviceToHost, st), "D2H");
        hip_ok(hipMemcpyAsync(h_mv + nb * 4, d_sad, nb * 4, hipMemcpyDeviceToHost, st), "D2H");
        hip_ok(hipStreamSynchronize(st), "sync");
        const int16_t* v = reinterpret_cast<const int16_t*>(h_mv);
        const uint32_t* s = reinterpret_cast<const uint32_t*>(h_mv + nb * 4);
        long long nonzero = 0, sdx = 0, sdy = 0, mx = 0;
        unsigned long long ssad = 0;
        for (size_t b = 0; b < nb; ++b) {
            const long long ax = std::abs(static_cast<int>(v[2 * b])), ay = std::abs(static_cast<int>(v[2 * b + 1]));
            nonzero += (ax | ay) != 0;
            sdx += ax; sdy += ay;
            mx = std::max(mx, std::max(ax, ay));
            ssad += s[b];
        }
        mv_records += std::string(mv_records.empty() ? "" : ",") + "\n    {\"idx\": " + std::to_string(pictures) + ", \"blocks\": " + std::to_string(nb) +
                      ", \"nonzero\": " + std::to_string(nonzero) + ", \"sum_abs_dx\": " + std::to_string(sdx) + ", \"sum_abs_dy\": " +
                      std::to_string(sdy) + ", \"max_abs\": " + std::to_string(mx) + ", \"sum_sad\": " + std::to_string(ssad) + "}";
    }
    // the summary line's tail and --mv-log's file; g supplies the coded size
    std::string finish_mc(const Geometry& g, hipStream_t st)
    {
        if (!arg.mc) return "";
        uint32_t moved = 0;
        if (d_moved) {
            hip_ok(hipMemcpyAsync(&moved, d_moved, sizeof(moved), hipMemcpyDeviceToHost, st), "D2H");
            hip_ok(hipStreamSynchronize(st), "sync");
        }
        if (!arg.mv_log.empty()) {
            const std::string text = "{\n  \"range\": " + std::to_string(arg.mc_range) + ",\n  \"lambda\": " + std::to_string(arg.mc_lambda) +
                                     ",\n  \"block\": 16,\n  \"width\": " + std::to_string(g.W) + ",\n  \"height\": " + std::to_string(g.H) +
                                     ",\n  \"pictures\": [" + mv_records + (mv_records.empty() ? "" : "\n  ") + "]\n}\n";
            FILE* lf = fopen(arg.mv_log.c_str(), "wb");
            if (!lf || fwrite(text.data(), 1, text.size(), lf) != text.size() || fclose(lf) != 0) die("cannot write " + arg.mv_log);
        }
        return ", mc range " + std::to_string(arg.mc_range) + " lambda " + std::to_string(arg.mc_lambda) + " (" + std::to_string(moved) + " of " +
               std::to_string(searched * bh * bw) + " blocks moved)";
    }
    void destroy()
    {
        for (uint8_t* p : hist) {
            if (p) hip_ok(hipFree(p), "hipFree");
        }
        for (void* p : {static_cast<void*>(comp), static_cast<void*>(d_mv), static_cast<void*>(d_sad), static_cast<void*>(d_moved), d_ws}) {
            if (p) hip_ok(hipFree(p), "hipFree");
        }
        if (h_mv) hip_ok(hipHostFree(h_mv), "hipHostFree");
        if (h_out) hip_ok(hipHostFree(h_out), "hipHostFree");
        if (file && fclose(file) != 0) die("cannot write " + arg.out);
        *this = Denoiser{};
    }
};

// --deinterlace MODE[:T] / --field-order / --deinterlace-out FILE (encode): what the flags alone decide is refused
// before a model is loaded
struct DeinterlaceArgs {
    bool on = false;
    bool field = false;            // field: two coded pictures a source frame; frame: one
    bool bff = false;              // --field-order bff, or a Y4M file's Ib
    int threshold = 10;
    std::string out;               // --deinterlace-out: the deinterlaced clip at the source size, raw
    const char* mode() const { return field ? "field" : "frame"; }
    const char* order() const { return bff ? "bff" : "tff"; }
};

DeinterlaceArgs deinterlace_args(const Args& a, bool encoding)
{
    DeinterlaceArgs d;
    if (!encoding) {
        for (const char* k : {"deinterlace", "field-order", "deinterlace-out"}) {
            if (a.has(k)) die(std::string("--") + k + " is an encoder flag");
        }
        return d;
    }
    if (!a.has("deinterlace")) {
        // --field-order belongs to --ivtc as well (ivtc_args reads it)
        if (a.has("field-order") && !a.has("ivtc")) die("--field-order needs --deinterlace or --ivtc");
        if (a.has("deinterlace-out")) die("--deinterlace-out needs --deinterlace");
        return d;
    }
    // "frame" or "field", then ":T" with a decimal integer in 0..64, nothing else
    const std::string s = a.str("deinterlace");
    const size_t colon = s.find(':');
    const std::string mode = s.substr(0, colon);
    bool good = mode == "frame" || mode == "field";
    if (good && colon != std::string::npos) {
        const std::string t = s.substr(colon + 1);
        good = !t.empty() && t.size() <= 2 && t.find_first_not_of("0123456789") == std::string::npos && atoi(t.c_str()) <= 64;
        if (good) d.threshold = atoi(t.c_str());
    }
    if (!good) die("--deinterlace must be frame or field, or either with :T, T an integer in 0..64, got " + s);
    d.field = mode == "field";
    if (a.has("field-order")) {
        const std::string o = a.str("field-order");
        if (o != "tff" && o != "bff") die("--field-order must be tff or bff, got " + o);
        d.bff = o == "bff";
    }
    const std::string type = a.str("src-type", "yuv420");
    if (is_rgb_name(type)) die("--deinterlace is for planar YUV sources: RGB sources are not deinterlaced yet");
    if (type == "nv12" || type == "p010" || type == "nv21") {
        die("--deinterlace is for planar YUV sources: " + type + " sources are not deinterlaced yet");
    }
    d.out = a.str("deinterlace-out");
    if (a.has("deinterlace-out") && (d.out.empty() || is_dash(d.out))) {
        die("--deinterlace-out needs a file name (not -: stdout is for the stream)");
    }
    d.on = true;
    return d;
}

// --deinterlace: the planes of a woven source frame through dcvc_deinterlace_planes, Y in one call, U and V in one call. The
// last two INPUT frames (behind the upload and the unpack) stay on the device in two buffers used in turn; in field mode a
// frame serves two pictures: its first field's (woven with the previous frame's second field), then its second field's.
struct Deinterlacer {
    DeinterlaceArgs arg;
    uint8_t* in[2] = {nullptr, nullptr};
    uint8_t* h_out = nullptr;      // pinned: --deinterlace-out's picture
    FILE* file = nullptr;
    int turn = 0, phase = 0;       // phase 1: the second picture of in[turn] is due
    long long frames = 0, pictures = 0;
    void create(const Geometry& g, const DeinterlaceArgs& d)
    {
        arg = d;
        for (uint8_t*& p : in) hip_ok(hipMalloc(&p, g.frame_bytes()), "hipMalloc");
        if (!arg.out.empty()) {
            hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_out), g.frame_bytes(), hipHostMallocDefault), "hipHostMalloc");
            file = fopen(arg.out.c_str(), "wb");
            if (!file) die("cannot write " + arg.out);
        }
    }
    bool wants_frame() const { return phase == 0; }
    // where the next source frame goes (planes Y, U, V back to back, u8 or u16 by the bit depth) when wants_frame()
    uint8_t* next_input()
    {
        ++frames;
        return in[turn];
    }
    // the next picture of the frame in in[turn] -> dst
    void run(const Geometry& g, uint8_t* dst, hipStream_t st)
    {
        const int es = g.hbd() ? 2 : 1, dt = g.hbd() ? DCVC_SAMPLE_U16 : DCVC_SAMPLE_U8;
        const long long ny = static_cast<long long>(g.H) * g.W, nc = static_cast<long long>(g.Hc()) * g.Wc();
        const int p0 = arg.bff ? 1 : 0, keep = phase == 0 ? p0 : 1 - p0, weave = arg.field && phase == 0 ? 1 : 0;
        const uint8_t* cur = in[turn];
        const uint8_t* prev = frames > 1 ? in[turn ^ 1] : nullptr;
        abi_ok(dcvc_deinterlace_planes(cur, g.W, ny, prev, g.W, ny, dst, g.W, ny, dt, g.bit_depth, g.H, g.W, 1, keep, weave, arg.threshold, st),
               "deinterlace (Y)");
        abi_ok(dcvc_deinterlace_planes(cur + ny * es, g.Wc(), nc, prev ? prev + ny * es : nullptr, g.Wc(), nc, dst + ny * es, g.Wc(), nc, dt,
                                       g.bit_depth, g.Hc(), g.Wc(), 2, keep, weave, arg.threshold, st), "deinterlace (U, V)");
        if (file) {
            hip_ok(hipMemcpyAsync(h_out, dst, g.frame_bytes(), hipMemcpyDeviceToHost, st), "D2H");
            hip_ok(hipStreamSynchronize(st), "sync");
            if (fwrite(h_out, 1, g.frame_bytes(), file) != g.frame_bytes()) die("cannot write " + arg.out);
        }
        ++pictures;
        if (arg.field && phase == 0) {
            phase = 1;
        } else {
            phase = 0;
            turn ^= 1;
        }
    }
    void destroy()
    {
        for (uint8_t* p : in) {
            if (p) hip_ok(hipFree(p), "hipFree");
        }
        if (h_out) hip_ok(hipHostFree(h_out), "hipHostFree");
        if (file && fclose(file) != 0) die("cannot write " + arg.out);
        *this = Deinterlacer{};
    }
};

// --ivtc film|match[:CTHRESH[:MI[:T]]] / --ivtc-out FILE / --ivtc-log FILE (encode): what the flags alone decide is
// refused before a model is loaded
struct IvtcArgs {
    bool on = false;
    bool film = false;             // film: matching and decimation with cycle 5; match: matching only
    bool bff = false;              // --field-order bff, or a Y4M file's Ib
    int cthresh = 9, mi = 80;      // the TIVTC defaults for a 256-sample block
    int threshold = 10;            // the deinterlacer's, for combed frames
    std::string out;               // --ivtc-out: the pictures at the source size, raw
    std::string log;               // --ivtc-log: the words and decisions of every source frame, JSON
    const char* mode() const { return film ? "film" : "match"; }
    const char* order() const { return bff ? "bff" : "tff"; }
};

IvtcArgs ivtc_args(const Args& a, bool encoding)
{
    IvtcArgs d;
    if (!encoding) {
        for (const char* k : {"ivtc", "ivtc-out", "ivtc-log"}) {
            if (a.has(k)) die(std::string("--") + k + " is an encoder flag");
        }
        return d;
    }
    if (!a.has("ivtc")) {
        for (const char* k : {"ivtc-out", "ivtc-log"}) {
            if (a.has(k)) die(std::string("--") + k + " needs --ivtc");
        }
        return d;
    }
    if (a.has("deinterlace")) die("--ivtc and --deinterlace exclude each other: --ivtc deinterlaces the frames it finds combed itself");
    // "film" or "match", then up to three ":N" with decimal integers: CTHRESH 0..255, MI 0..512, T 0..64
    const std::string s = a.str("ivtc");
    std::vector<std::string> parts;
    for (size_t at = 0;;) {
        const size_t colon = s.find(':', at);
        parts.push_back(s.substr(at, colon == std::string::npos ? std::string::npos : colon - at));
        if (colon == std::string::npos) break;
        at = colon + 1;
    }
    bool good = (parts[0] == "film" || parts[0] == "match") && parts.size() <= 4;
    const int top[3] = {255, 512, 64};
    int* into[3] = {&d.cthresh, &d.mi, &d.threshold};
    for (size_t k = 1; good && k < parts.size(); ++k) {
        const std::string& t = parts[k];
        good = !t.empty() && t.size() <= 3 && t.find_first_not_of("0123456789") == std::string::npos && atoi(t.c_str()) <= top[k - 1];
        if (good) *into[k - 1] = atoi(t.c_str());
    }
    if (!good) {
        die("--ivtc must be film or match, or either with :CTHRESH[:MI[:T]], integers in 0..255, 0..512 and 0..64, got " + s);
    }
    d.film = parts[0] == "film";
    if (a.has("field-order")) {
        const std::string o = a.str("field-order");
        if (o != "tff" && o != "bff") die("--field-order must be tff or bff, got " + o);
        d.bff = o == "bff";
    }
    const std::string type = a.str("src-type", "yuv420");
    if (is_rgb_name(type)) die("--ivtc is for planar YUV sources: RGB sources are not deinterlaced yet");
    if (type == "nv12" || type == "p010" || type == "nv21") {
        die("--ivtc is for planar YUV sources: " + type + " sources are not deinterlaced yet");
    }
    d.out = a.str("ivtc-out");
    if (a.has("ivtc-out") && (d.out.empty() || is_dash(d.out))) die("--ivtc-out needs a file name (not -: stdout is for the stream)");
    d.log = a.str("ivtc-log");
    if (a.has("ivtc-log") && (d.log.empty() || is_dash(d.log))) die("--ivtc-log needs a file name (not -: stdout is for the stream)");
    d.on = true;
    return d;
}

// --ivtc: the last cycle + 1 source frames (behind the upload and the unpack) stay on the device in a ring. A cycle of frames is
// read, every frame measured against its predecessor (dcvc_field_match on the luma planes, the eight words copied to the
// host) and pushed (dcvc_ivtc_push); a complete cycle of film mode then loses the frame dcvc_ivtc_drop names, and the frames that
// stay are served in order: woven (dcvc_weave_fields) from their own first field and the second field of the match, or, when
// combed, deinterlaced as --deinterlace frame:T would. match mode is a cycle of one frame without a drop.
struct IvtcStage {
    struct Frame {
        unsigned long long words[8];
        int match = 0;
        bool combed = false, dropped = false;
    };
    static constexpr int kCycle = 5;
    IvtcArgs arg;
    std::vector<uint8_t*> ring;
    unsigned long long* words = nullptr;       // device: dcvc_field_match's eight words
    unsigned long long* h_words = nullptr;     // pinned
    uint8_t* h_out = nullptr;                  // pinned: --ivtc-out's picture
    FILE* file = nullptr;
    dcvc_ivtc* decide = nullptr;
    std::vector<Frame> log;                    // every source frame read
    std::vector<long long> queue;              // the source frames that wait to be served, in order
    size_t served = 0;                         // ... and how many of them are
    long long pictures = 0, matched_prev = 0, deinterlaced = 0, dropped = 0;
    int cycle() const { return arg.film ? kCycle : 1; }
    long long frames() const { return static_cast<long long>(log.size()); }
    bool pending() const { return served < queue.size(); }
    void create(const Geometry& g, const IvtcArgs& d)
    {
        arg = d;
        ring.assign(static_cast<size_t>(cycle() + 1), nullptr);
        for (uint8_t*& p : ring) hip_ok(hipMalloc(&p, g.frame_bytes()), "hipMalloc");
        hip_ok(hipMalloc(&words, 8 * sizeof(unsigned long long)), "hipMalloc");
        hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_words), 8 * sizeof(unsigned long long), hipHostMallocDefault), "hipHostMalloc");
        decide = dcvc_ivtc_create(arg.film ? kCycle : 0, arg.mi);
        if (!decide) die(std::string("ivtc: ") + dcvc_last_error());
        if (!arg.out.empty()) {
            hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_out), g.frame_bytes(), hipHostMallocDefault), "hipHostMalloc");
            file = fopen(arg.out.c_str(), "wb");
            if (!file) die("cannot write " + arg.out);
        }
    }
    uint8_t* slot(long long f) const { return ring[static_cast<size_t>(f) % ring.size()]; }
    // where the next source frame goes (planes Y, U, V back to back, u8 or u16 by the bit depth)
    uint8_t* next_input() const { return slot(frames()); }
    // the frame next_input() took: measured against its predecessor and pushed; waits for the stream (the words are needed here,
    // and the pinned memory the upload read is free again)
    void measure(const Geometry& g, hipStream_t st)
    {
        const long long f = frames();
        const int dt = g.hbd() ? DCVC_SAMPLE_U16 : DCVC_SAMPLE_U8;
        abi_ok(dcvc_field_match(slot(f), g.W, f > 0 ? slot(f - 1) : nullptr, g.W, dt, g.bit_depth, g.H, g.W, arg.bff ? 1 : 0, arg.cthresh, words, st),
               "field_match");
        hip_ok(hipMemcpyAsync(h_words, words, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st), "D2H");
        hip_ok(hipStreamSynchronize(st), "sync");
        Frame fr;
        uint64_t m[8];
        for (int k = 0; k < 8; ++k) m[k] = fr.words[k] = h_words[k];
        const int r = dcvc_ivtc_push(decide, static_cast<int>(f), f > 0 ? 1 : 0, m);
        abi_ok(r, "ivtc");
        fr.match = r & 1;
        fr.combed = (r & 2) != 0;
        log.push_back(fr);
    }
    // the `got` frames read last are the cycle: a complete one of film mode loses the frame dcvc_ivtc_drop names
    void close_cycle(int got)
    {
        queue.clear();
        served = 0;
        const long long f0 = frames() - got;
        const int drop = arg.film && got == kCycle ? dcvc_ivtc_drop(decide) : -1;
        for (int k = 0; k < got; ++k) {
            if (k == drop) {
                log[static_cast<size_t>(f0 + k)].dropped = true;
                ++dropped;
            } else {
                queue.push_back(f0 + k);
            }
        }
    }
    // the next frame that waits -> dst
    void serve(const Geometry& g, uint8_t* dst, hipStream_t st)
    {
        const long long f = queue[served++];
        const Frame& fr = log[static_cast<size_t>(f)];
        const int es = g.hbd() ? 2 : 1, dt = g.hbd() ? DCVC_SAMPLE_U16 : DCVC_SAMPLE_U8, first = arg.bff ? 1 : 0;
        const long long ny = static_cast<long long>(g.H) * g.W, nc = static_cast<long long>(g.Hc()) * g.Wc();
        const uint8_t* cur = slot(f);
        const uint8_t* prev = f > 0 ? slot(f - 1) : nullptr;
        if (fr.combed) {
            abi_ok(dcvc_deinterlace_planes(cur, g.W, ny, prev, g.W, ny, dst, g.W, ny, dt, g.bit_depth, g.H, g.W, 1, first, 0, arg.threshold, st),
                   "deinterlace (Y)");
            abi_ok(dcvc_deinterlace_planes(cur + ny * es, g.Wc(), nc, prev ? prev + ny * es : nullptr, g.Wc(), nc, dst + ny * es, g.Wc(), nc, dt,
                                           g.bit_depth, g.Hc(), g.Wc(), 2, first, 0, arg.threshold, st), "deinterlace (U, V)");
            ++deinterlaced;
        } else {
            const uint8_t* second = fr.match ? prev : cur;
            abi_ok(dcvc_weave_fields(cur, g.W, ny, second, g.W, ny, dst, g.W, ny, dt, g.H, g.W, 1, first, st), "weave_fields (Y)");
            abi_ok(dcvc_weave_fields(cur + ny * es, g.Wc(), nc, second + ny * es, g.Wc(), nc, dst + ny * es, g.Wc(), nc, dt, g.Hc(), g.Wc(), 2,
                                     first, st), "weave_fields (U, V)");
        }
        if (fr.match) ++matched_prev;
        if (file) {
            hip_ok(hipMemcpyAsync(h_out, dst, g.frame_bytes(), hipMemcpyDeviceToHost, st), "D2H");
            hip_ok(hipStreamSynchronize(st), "sync");
            if (fwrite(h_out, 1, g.frame_bytes(), file) != g.frame_bytes()) die("cannot write " + arg.out);
        }
        ++pictures;
    }
    void write_log() const
    {
        if (arg.log.empty()) return;
        std::string js = std::string("{\"mode\": \"") + arg.mode() + "\", \"field_order\": \"" + arg.order() + "\", \"cthresh\": " +
                         std::to_string(arg.cthresh) + ", \"mi\": " + std::to_string(arg.mi) + ", \"threshold\": " + std::to_string(arg.threshold) +
                         ", \"pictures\": " + std::to_string(pictures) + ", \"frames\": [";
        for (size_t f = 0; f < log.size(); ++f) {
            js += f ? ",\n  {\"words\": [" : "\n  {\"words\": [";
            for (int k = 0; k < 8; ++k) js += (k ? ", " : "") + std::to_string(log[f].words[k]);
            js += std::string("], \"match\": \"") + (log[f].match ? "p" : "c") + "\", \"combed\": " + (log[f].combed ? "true" : "false") +
                  ", \"dropped\": " + (log[f].dropped ? "true" : "false") + "}";
        }
        js += "\n]}\n";
        FILE* lf = fopen(arg.log.c_str(), "wb");
        if (!lf || fwrite(js.data(), 1, js.size(), lf) != js.size() || fclose(lf) != 0) die("cannot write " + arg.log);
    }
    void destroy()
    {
        for (uint8_t* p : ring) {
            if (p) hip_ok(hipFree(p), "hipFree");
        }
        if (words) hip_ok(hipFree(words), "hipFree");
        if (h_words) hip_ok(hipHostFree(h_words), "hipHostFree");
        if (h_out) hip_ok(hipHostFree(h_out), "hipHostFree");
        if (decide) dcvc_ivtc_destroy(decide);
        if (file && fclose(file) != 0) die("cannot write " + arg.out);
        *this = IvtcStage{};
    }
};

// ------------------------------------------------------------------------------------ black bars
// "A:B:C" -> three integers in 0..max
bool parse_triple(const std::string& s, unsigned long long max, int (&v)[3])
{
    size_t at = 0;
    for (int k = 0; k < 3; ++k) {
        const size_t colon = k < 2 ? s.find(':', at) : s.size();
        unsigned long long n = 0;
        if (colon == std::string::npos || !parse_uint(s.substr(at, colon - at), max, n)) return false;
        v[k] = static_cast<int>(n);
        at = colon + 1;
    }
    return true;
}

// "WxH+X+Y" -> the four, each at most kMaxPictureSide
bool parse_window(const std::string& s, int& w, int& h, int& x, int& y)
{
    const size_t ex = s.find('x'), p1 = s.find('+'), p2 = p1 == std::string::npos ? p1 : s.find('+', p1 + 1);
    if (ex == std::string::npos || p2 == std::string::npos || ex > p1) return false;
    unsigned long long v[4];
    const std::string part[4] = {s.substr(0, ex), s.substr(ex + 1, p1 - ex - 1), s.substr(p1 + 1, p2 - p1 - 1), s.substr(p2 + 1)};
    for (int k = 0; k < 4; ++k) {
        if (!parse_uint(part[k], kMaxPictureSide, v[k])) return false;
    }
    w = static_cast<int>(v[0]); h = static_cast<int>(v[1]); x = static_cast<int>(v[2]); y = static_cast<int>(v[3]);
    return true;
}

// the chroma planes' subsampling of a picture against its luma plane: 2, 2 for 4:2:0; 2, 1 for 4:2:2; 1, 1 for 4:4:4
int chroma_sx(const Geometry& g) { return g.W / g.Wc(); }
int chroma_sy(const Geometry& g) { return g.H / g.Hc(); }

// a window of the planes (Y, U, V back to back) of a `from` picture -> the planes of a `to` picture, the window's origin at
// (x, y) of `from` in luma samples (negative: `to` is the larger one and `from` lies at (-x, -y) in it): dcvc_window_planes,
// Y in one call, U and V in one call
void window_picture(const Geometry& from, const uint8_t* src, const Geometry& to, uint8_t* dst, int x, int y, const int (&fill)[3], hipStream_t st)
{
    const int es = from.hbd() ? 2 : 1, dt = from.hbd() ? DCVC_SAMPLE_U16 : DCVC_SAMPLE_U8;
    const long long fy = static_cast<long long>(from.H) * from.W, fc = static_cast<long long>(from.Hc()) * from.Wc();
    const long long ty = static_cast<long long>(to.H) * to.W, tc = static_cast<long long>(to.Hc()) * to.Wc();
    abi_ok(dcvc_window_planes(src, from.W, fy, from.H, from.W, dst, to.W, ty, to.H, to.W, dt, 1, x, y, fill, st), "window (Y)");
    abi_ok(dcvc_window_planes(src + fy * es, from.Wc(), fc, from.Hc(), from.Wc(), dst + ty * es, to.Wc(), tc, to.Hc(), to.Wc(), dt, 2,
                              x / chroma_sx(from), y / chroma_sy(from), fill + 1, st), "window (U, V)");
}

// --crop auto[:LIMIT[:FRAC[:MINBAR[:N]]]] | WxH+X+Y / --crop-log FILE / --crop-out FILE / --crop-fill Y:U:V (encode):
// what the flags alone decide is refused before a model is loaded
struct CropArgs {
    bool on = false, automatic = false;
    int limit = 24, frac = 4, min_bar = 8, probes = 16;      // nobody has tuned these for this project
    int x = 0, y = 0, w = 0, h = 0;                          // the window: manual, or what the detection found
    bool fill_given = false;
    int fill[3] = {16, 128, 128};                            // at the source's depth once that is known
    std::string log, out;
    const char* mode() const { return automatic ? "auto" : "manual"; }
};

CropArgs crop_args(const Args& a, bool encoding)
{
    CropArgs c;
    if (!encoding) {
        for (const char* k : {"crop", "crop-log", "crop-out", "crop-fill"}) {
            if (a.has(k)) die(std::string("--") + k + " is an encoder flag: decode puts the bars back with --uncrop FILE or --pad SWxSH+X+Y");
        }
        return c;
    }
    for (const char* k : {"uncrop", "pad", "pad-fill"}) {
        if (a.has(k)) die(std::string("--") + k + " is a decoder flag: encode drops the bars with --crop");
    }
    if (!a.has("crop")) {
        for (const char* k : {"crop-log", "crop-out", "crop-fill"}) {
            if (a.has(k)) die(std::string("--") + k + " needs --crop");
        }
        return c;
    }
    const std::string s = a.str("crop");
    const char* form = "--crop must be auto, auto:LIMIT[:FRAC[:MINBAR[:N]]] with integers in 0..255, 0..255, 0..4096 and 1..256, or WxH+X+Y, got ";
    if (s.rfind("auto", 0) == 0) {
        std::vector<std::string> parts;
        for (size_t at = 0;;) {
            const size_t colon = s.find(':', at);
            parts.push_back(s.substr(at, colon == std::string::npos ? std::string::npos : colon - at));
            if (colon == std::string::npos) break;
            at = colon + 1;
        }
        bool good = parts[0] == "auto" && parts.size() <= 5;
        const unsigned long long top[4] = {255, 255, 4096, 256};
        int* into[4] = {&c.limit, &c.frac, &c.min_bar, &c.probes};
        for (size_t k = 1; good && k < parts.size(); ++k) {
            unsigned long long v = 0;
            good = parse_uint(parts[k], top[k - 1], v) && (k < 4 || v >= 1);
            if (good) *into[k - 1] = static_cast<int>(v);
        }
        if (!good) die(form + s);
        c.automatic = true;
    } else if (!parse_window(s, c.w, c.h, c.x, c.y)) {
        die(form + s);
    }
    const std::string type = a.str("src-type", "yuv420");
    if (is_rgb_name(type)) die("--crop is for planar YUV sources: RGB sources are not cropped yet");
    if (type == "nv12" || type == "p010" || type == "nv21") die("--crop is for planar YUV sources: " + type + " sources are not cropped yet");
    for (const char* k : {"crop-log", "crop-out"}) {
        if (a.has(k) && (a.str(k).empty() || is_dash(a.str(k)))) die(std::string("--") + k + " needs a file name (not -: stdout is for the stream)");
    }
    c.log = a.str("crop-log");
    c.out = a.str("crop-out");
    if (a.has("crop-fill")) {
        if (!parse_triple(a.str("crop-fill"), 65535, c.fill)) die("--crop-fill must be Y:U:V, three sample values, got " + a.str("crop-fill"));
        c.fill_given = true;
    }
    if (c.automatic && (is_dash(a.str("i")) || names_a_pipe(a.str("i")))) die("--crop auto needs a seekable source; give --crop WxH+X+Y");
    c.on = true;
    return c;
}

// one probed picture of --crop auto
struct CropProbe {
    long long idx = 0;
    bool voted = false;
    int top = 0, bottom = 0, left = 0, right = 0;
};

// --crop: the window is settled before the first picture is coded - checked (manual) or found (auto: N' = min(N, M) of the M
// source frames the run will read, frame ((2k + 1) M) / (2 N') for k = 0 .. N' - 1, each read with pread, uploaded, unpacked when
// it is a wire type, measured by dcvc_crop_stats and pushed to dcvc_cropdet_*). Then every source picture's upload (and unpack)
// lands in a buffer of the file's size, and dcvc_window_planes writes the window where the upload would have landed.
struct CropStage {
    CropArgs arg;
    bool active = false;           // the window is smaller than the picture: there is something to cut
    int ax = 2, ay = 2;
    std::vector<CropProbe> probes;
    int votes = 0;
    WireStage wsf;                 // a wire format's pictures at the FILE's size
    uint8_t* full = nullptr;       // the file's picture on the device: planes Y, U, V
    uint8_t* h_in = nullptr;       // pinned: the file's picture
    uint8_t* h_out = nullptr;      // pinned: --crop-out's picture
    FILE* file = nullptr;
    long long pictures = 0;
    // the source type's alignment; the codec takes even sides only, so a 4:4:4 or 4:2:2 window is even all the same
    void align(const Geometry& gf, bool fields)
    {
        ax = std::max(chroma_sx(gf), 2);
        ay = std::max(chroma_sy(gf), 2) * (fields ? 2 : 1);
    }
    void check_manual(const Geometry& gf) const
    {
        const std::string w = std::to_string(arg.w) + "x" + std::to_string(arg.h) + "+" + std::to_string(arg.x) + "+" + std::to_string(arg.y);
        if (arg.w < 1 || arg.h < 1) die("--crop " + w + ": the window's sides must be positive");
        if (arg.x + arg.w > gf.W || arg.y + arg.h > gf.H) {
            die("--crop " + w + " does not lie inside the " + std::to_string(gf.W) + "x" + std::to_string(gf.H) + " picture");
        }
        if (arg.x % ax || arg.w % ax || arg.y % ay || arg.h % ay) {
            die("--crop " + w + ": offsets and sides must be multiples of " + std::to_string(ax) + " (horizontal) and " + std::to_string(ay) +
                " (vertical) for this source" + (ay > 2 ? " (field rows: --deinterlace / --ivtc double the vertical step)" : ""));
        }
    }
    // auto: M = the source frames the run will read
    void detect(PictureFile& f, const Geometry& gf, long long M)
    {
        allocate(gf);
        if (gf.H % ay || gf.W % ax) {
            die("--crop auto: the " + std::to_string(gf.W) + "x" + std::to_string(gf.H) + " picture is no multiple of the window's step, " +
                std::to_string(ax) + "x" + std::to_string(ay));
        }
        dcvc_cropdet* det = dcvc_cropdet_create(gf.H, gf.W, arg.frac, arg.min_bar, ax, ay);
        if (!det) die(std::string("--crop auto: ") + dcvc_last_error());
        const long long n = std::min<long long>(arg.probes, M);
        const std::vector<long long> at = f.offsets(gf.file_bytes(), M);
        const size_t words = static_cast<size_t>(gf.H + gf.W);
        hipStream_t st = nullptr;
        uint32_t* counts = nullptr;
        uint32_t* h_counts = nullptr;
        hip_ok(hipStreamCreate(&st), "hipStreamCreate");
        hip_ok(hipMalloc(&counts, words * sizeof(uint32_t)), "hipMalloc");
        hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_counts), words * sizeof(uint32_t), hipHostMallocDefault), "hipHostMalloc");
        const int dt = gf.hbd() ? DCVC_SAMPLE_U16 : DCVC_SAMPLE_U8;
        for (long long k = 0; k < n; ++k) {
            CropProbe p;
            p.idx = ((2 * k + 1) * M) / (2 * n);
            size_t got = 0;
            while (got < gf.file_bytes()) {
                const ssize_t r = pread(f.fd, h_in + got, gf.file_bytes() - got, at[static_cast<size_t>(p.idx)] + static_cast<long long>(got));
                if (r < 0 && errno == EINTR) continue;
                if (r <= 0) die("cannot read picture " + std::to_string(p.idx + 1) + " of " + f.path);
                got += static_cast<size_t>(r);
            }
            if (gf.wire >= 0) wsf.upload(gf, full, st, h_in);
            else hip_ok(hipMemcpyAsync(full, h_in, gf.frame_bytes(), hipMemcpyHostToDevice, st), "H2D");
            abi_ok(dcvc_crop_stats(full, gf.W, dt, gf.bit_depth, gf.H, gf.W, arg.limit, counts, st), "crop_stats");
            hip_ok(hipMemcpyAsync(h_counts, counts, words * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H");
            hip_ok(hipStreamSynchronize(st), "sync");
            const int voted = dcvc_cropdet_push(det, h_counts);
            abi_ok(voted, "cropdet");
            p.voted = voted == 1;
            if (p.voted) {
                // the picture's own rectangle for the log: the same words through a detector of its own, nothing dropped or rounded
                dcvc_cropdet* one = dcvc_cropdet_create(gf.H, gf.W, arg.frac, 0, 1, 1);
                if (!one) die(std::string("--crop auto: ") + dcvc_last_error());
                int x = 0, y = 0, w = 0, h = 0;
                abi_ok(dcvc_cropdet_push(one, h_counts), "cropdet");
                abi_ok(dcvc_cropdet_result(one, &x, &y, &w, &h), "cropdet");
                dcvc_cropdet_destroy(one);
                p.top = y; p.bottom = y + h - 1; p.left = x; p.right = x + w - 1;
            }
            probes.push_back(p);
        }
        votes = dcvc_cropdet_result(det, &arg.x, &arg.y, &arg.w, &arg.h);
        abi_ok(votes, "cropdet");
        dcvc_cropdet_destroy(det);
        active = arg.w != gf.W || arg.h != gf.H;
        hip_ok(hipFree(counts), "hipFree");
        hip_ok(hipHostFree(h_counts), "hipHostFree");
        hip_ok(hipStreamDestroy(st), "hipStreamDestroy");
    }
    // what needs no device: the step, the fill values, a manual window's check. gf: the file's pictures.
    void create(const CropArgs& c, const Geometry& gf, bool fields)
    {
        arg = c;
        align(gf, fields);
        if (!arg.fill_given) {
            for (int& v : arg.fill) v <<= gf.bit_depth - 8;
        }
        for (int v : arg.fill) {
            if (v > (1 << gf.bit_depth) - 1) die("--crop-fill: " + std::to_string(v) + " is no sample of " + std::to_string(gf.bit_depth) + " bits");
        }
        if (!arg.automatic) {
            check_manual(gf);
            active = arg.w != gf.W || arg.h != gf.H;
        }
    }
    // the buffers of the file's size: in front of the detection, or of the first picture
    void allocate(const Geometry& gf)
    {
        if (full) return;
        hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_in), gf.file_bytes(), hipHostMallocDefault), "hipHostMalloc");
        hip_ok(hipMalloc(&full, gf.frame_bytes()), "hipMalloc");
        wsf.create(gf);
    }
    // --crop-out opens once the window, and with it the pictures' size, is known
    void open_out(const Geometry& gs)
    {
        if (arg.out.empty()) return;
        hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_out), gs.frame_bytes(), hipHostMallocDefault), "hipHostMalloc");
        file = fopen(arg.out.c_str(), "wb");
        if (!file) die("cannot write " + arg.out);
    }
    // the file's picture in pinned memory at h -> the window's planes at dst, where the upload of a picture of that size lands
    void upload(const Geometry& gf, const Geometry& gs, uint8_t* dst, const uint8_t* h, hipStream_t st)
    {
        if (gf.wire >= 0) wsf.upload(gf, full, st, h);
        else hip_ok(hipMemcpyAsync(full, h, gf.frame_bytes(), hipMemcpyHostToDevice, st), "H2D");
        window_picture(gf, full, gs, dst, arg.x, arg.y, arg.fill, st);
    }
    // --crop-out: the source picture as everything behind the stage sees it, the carrier's raw layout
    void written(const Geometry& gs, const uint8_t* dst, hipStream_t st)
    {
        ++pictures;
        if (!file) return;
        hip_ok(hipMemcpyAsync(h_out, dst, gs.frame_bytes(), hipMemcpyDeviceToHost, st), "D2H");
        hip_ok(hipStreamSynchronize(st), "sync");
        if (fwrite(h_out, 1, gs.frame_bytes(), file) != gs.frame_bytes()) die("cannot write " + arg.out);
    }
    void write_log(const Geometry& gf, const std::string& type_name) const
    {
        if (arg.log.empty()) return;
        auto num_or_null = [&](int v) { return arg.automatic ? std::to_string(v) : std::string("null"); };
        std::string js = std::string("{\"mode\": \"") + arg.mode() + "\", \"limit\": " + num_or_null(arg.limit) + ", \"frac\": " + num_or_null(arg.frac) +
                         ", \"min_bar\": " + num_or_null(arg.min_bar) + ", \"source_width\": " + std::to_string(gf.W) + ", \"source_height\": " +
                         std::to_string(gf.H) + ", \"src_type\": \"" + type_name + "\", \"chroma_format\": \"" + chroma_name(gf) +
                         "\", \"bit_depth\": " + std::to_string(gf.bit_depth) + ", \"probes\": [";
        for (size_t i = 0; i < probes.size(); ++i) {
            const CropProbe& p = probes[i];
            auto side = [&](int v) { return p.voted ? std::to_string(v) : std::string("null"); };
            js += std::string(i ? ", " : "") + "{\"idx\": " + std::to_string(p.idx) + ", \"voted\": " + (p.voted ? "true" : "false") + ", \"top\": " +
                  side(p.top) + ", \"bottom\": " + side(p.bottom) + ", \"left\": " + side(p.left) + ", \"right\": " + side(p.right) + "}";
        }
        js += "], \"votes\": " + std::to_string(votes) + ", \"window\": {\"x\": " + std::to_string(arg.x) + ", \"y\": " + std::to_string(arg.y) +
              ", \"width\": " + std::to_string(arg.w) + ", \"height\": " + std::to_string(arg.h) + "}, \"fill\": [" + std::to_string(arg.fill[0]) + ", " +
              std::to_string(arg.fill[1]) + ", " + std::to_string(arg.fill[2]) + "]}\n";
        FILE* lf = fopen(arg.log.c_str(), "wb");
        if (!lf || fwrite(js.data(), 1, js.size(), lf) != js.size() || fclose(lf) != 0) die("cannot write " + arg.log);
    }
    void destroy()
    {
        wsf.destroy();
        if (full) hip_ok(hipFree(full), "hipFree");
        if (h_in) hip_ok(hipHostFree(h_in), "hipHostFree");
        if (h_out) hip_ok(hipHostFree(h_out), "hipHostFree");
        if (file && fclose(file) != 0) die("cannot write " + arg.out);
        *this = CropStage{};
    }
};

// --uncrop crop.json | --pad SWxSH+X+Y [--pad-fill Y:U:V] (decode): what the flags alone decide is refused before a
// model is loaded
struct PadArgs {
    bool on = false, from_file = false;
    std::string flag;              // the one that was given, for messages
    int W = 0, H = 0, x = 0, y = 0;            // the source's size and where the window lies in it
    int w = 0, h = 0;                          // --uncrop: the window's size
    bool fill_given = false;
    int fill[3] = {16, 128, 128};
    int bit_depth = 0;                         // --uncrop: what the log says of the pictures
    std::string chroma;
};

PadArgs pad_args(const Args& a)
{
    PadArgs p;
    if (a.has("uncrop") && a.has("pad")) die("--uncrop and --pad: exactly one of them may be given");
    if (!a.has("uncrop") && !a.has("pad")) {
        if (a.has("pad-fill")) die("--pad-fill needs --uncrop or --pad");
        return p;
    }
    p.flag = a.has("uncrop") ? "--uncrop" : "--pad";
    if (!a.has("o") && !a.has("hash-log") && !a.has("verify-hash")) {
        die(p.flag + " changes what -o writes and the hashes cover, nothing else: it needs -o, --hash-log or --verify-hash");
    }
    const std::string type = a.str("src-type", "yuv420");
    if (type != "yuv420" && type != "yuv422" && type != "yuv444") die(p.flag + " is for planar YUV pictures: " + type + " pictures are not padded yet");
    if (a.has("pad")) {
        if (!parse_window(a.str("pad"), p.W, p.H, p.x, p.y) || p.W < 2 || p.H < 2) {
            die("--pad must be SWxSH+X+Y: the source's size and where the picture lies in it, got " + a.str("pad"));
        }
    } else {
        const std::string path = a.str("uncrop");
        std::ifstream f(path, std::ios::binary);
        if (path.empty() || !f) die("--uncrop: cannot open " + path);
        const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        std::function<void(const std::string&)> bad = [&](const std::string& why) { die("--uncrop: " + path + " is no crop log: " + why); };
        JsonReader rd{text, bad};
        const Json top = rd.value(0);
        rd.space();
        if (rd.at != text.size()) bad("text behind the value");
        if (top.kind != Json::Object) bad("no object");
        auto num = [&](const Json& o, const std::string& key, unsigned long long lo, unsigned long long hi) {
            const Json* v = o.get(key);
            unsigned long long n = 0;
            if (!v || v->kind != Json::Number || !parse_uint(v->text, hi, n) || n < lo) {
                bad("\"" + key + "\" must be an integer in " + std::to_string(lo) + ".." + std::to_string(hi));
            }
            return static_cast<int>(n);
        };
        p.W = num(top, "source_width", 2, kMaxPictureSide);
        p.H = num(top, "source_height", 2, kMaxPictureSide);
        p.bit_depth = num(top, "bit_depth", 8, 16);
        const Json* cf = top.get("chroma_format");
        if (!cf || cf->kind != Json::String || (cf->text != "yuv420" && cf->text != "yuv422" && cf->text != "yuv444")) {
            bad("\"chroma_format\" must be yuv420, yuv422 or yuv444");
        }
        p.chroma = cf->text;
        const Json* win = top.get("window");
        if (!win || win->kind != Json::Object) bad("\"window\" must be an object");
        p.x = num(*win, "x", 0, kMaxPictureSide);
        p.y = num(*win, "y", 0, kMaxPictureSide);
        p.w = num(*win, "width", 2, kMaxPictureSide);
        p.h = num(*win, "height", 2, kMaxPictureSide);
        if (p.x + p.w > p.W || p.y + p.h > p.H) bad("the window does not lie inside the source");
        const Json* fl = top.get("fill");
        if (!fl || fl->kind != Json::Array || fl->items.size() != 3) bad("\"fill\" must be a list of 3");
        for (size_t k = 0; k < 3; ++k) {
            unsigned long long n = 0;
            if (fl->items[k].kind != Json::Number || !parse_uint(fl->items[k].text, 65535, n)) bad("\"fill\" holds integers in 0..65535");
            p.fill[k] = static_cast<int>(n);
        }
        p.fill_given = true;
        p.from_file = true;
    }
    if (a.has("pad-fill")) {
        if (!parse_triple(a.str("pad-fill"), 65535, p.fill)) die("--pad-fill must be Y:U:V, three sample values, got " + a.str("pad-fill"));
        p.fill_given = true;
    }
    p.on = true;
    return p;
}

// the log against the run's pictures, once their type and depth are settled (a Y4M --ref may supply them)
void pad_check_run(const PadArgs& p, const char* type, int depth)
{
    const std::string t = type;
    if (t != "yuv420" && t != "yuv422" && t != "yuv444") die(p.flag + " is for planar YUV pictures: " + t + " pictures are not padded yet");
    if (p.from_file && (p.bit_depth != depth || p.chroma != t)) {
        die("--uncrop: the log describes " + p.chroma + " pictures of " + std::to_string(p.bit_depth) + " bits, this run's are " + t + " of " +
            std::to_string(depth) + " bits");
    }
}

// decode: the output picture (planes Y, U, V back to back, behind the conversion, --out-size and the grain) -> the picture at
// the source's size in a buffer of the stage's own, the bars at the fill values: what -o, --hash-log and --verify-hash see. The
// metrics read the unpadded picture.
struct PadStage {
    PadArgs arg;
    Geometry g;                    // the padded picture's
    uint8_t* out = nullptr;
    uint8_t* h_out = nullptr;      // pinned
    // og: the picture arriving at the stage
    void create(const PadArgs& p, const Geometry& og)
    {
        destroy();                 // a stream may switch parameter sets
        arg = p;
        const std::string size = std::to_string(og.W) + "x" + std::to_string(og.H);
        if (og.rgb || og.wire >= 0 || (og.pix() && og.pix_fmt != DCVC_PIX_YUV422P && og.pix_fmt != DCVC_PIX_YUV444P)) {
            die(arg.flag + " is for planar YUV pictures: these pictures are not padded yet");
        }
        if (arg.from_file) {
            if (arg.w != og.W || arg.h != og.H) {
                die("--uncrop: the log's window is " + std::to_string(arg.w) + "x" + std::to_string(arg.h) + ", the pictures arriving are " + size);
            }
            if (arg.bit_depth != og.bit_depth || arg.chroma != chroma_name(og)) {
                die("--uncrop: the log describes " + arg.chroma + " pictures of " + std::to_string(arg.bit_depth) + " bits, this run's are " +
                    chroma_name(og) + " of " + std::to_string(og.bit_depth) + " bits");
            }
        }
        if (arg.x + og.W > arg.W || arg.y + og.H > arg.H) {
            die(arg.flag + ": a " + size + " picture at +" + std::to_string(arg.x) + "+" + std::to_string(arg.y) + " does not lie inside " +
                std::to_string(arg.W) + "x" + std::to_string(arg.H));
        }
        if ((arg.W & 1) || (arg.H & 1) || arg.x % chroma_sx(og) || arg.y % chroma_sy(og)) {
            die(arg.flag + ": the source's sides must be even and the offsets multiples of the chroma subsampling, " +
                std::to_string(chroma_sx(og)) + "x" + std::to_string(chroma_sy(og)));
        }
        if (!arg.fill_given) {
            for (int& v : arg.fill) v <<= og.bit_depth - 8;
        }
        for (int v : arg.fill) {
            if (v > (1 << og.bit_depth) - 1) die(arg.flag + ": fill value " + std::to_string(v) + " is no sample of " + std::to_string(og.bit_depth) + " bits");
        }
        g = geometry(arg.H, arg.W, false, og.bit_depth, og.pix_fmt);
        hip_ok(hipMalloc(&out, g.frame_bytes()), "hipMalloc");
        hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_out), g.frame_bytes(), hipHostMallocDefault), "hipHostMalloc");
    }
    const uint8_t* run(const Geometry& og, const uint8_t* shown, hipStream_t st)
    {
        window_picture(og, shown, g, out, -arg.x, -arg.y, arg.fill, st);
        return out;
    }
    void destroy()
    {
        if (out) hip_ok(hipFree(out), "hipFree");
        if (h_out) hip_ok(hipHostFree(h_out), "hipHostFree");
        *this = PadStage{};
    }
};

// --out-size: the output picture on the device and what measures it against the reference, all at the output size
struct ScaledOut {
    Resampler rs;
    uint8_t* out = nullptr;        // the resampled reconstruction: u8 or u16 planes
    uint8_t* ref = nullptr;        // the reference picture's planes
    uint8_t* h_out = nullptr;      // pinned
    uint8_t* h_ref = nullptr;      // pinned
    double* sse = nullptr;
    double* h_sse = nullptr;       // pinned
    double* ssim = nullptr;
    double* h_ssim = nullptr;      // pinned
    void* sse_ws = nullptr;
    long long sse_ws_bytes = 0;
    void* ssim_ws = nullptr;       // dcvc_msssim_range_ws's workspace: Y, then U and V, one after the other
    long long ssim_ws_bytes = 0;
    void create(const Geometry& from, const Geometry& to, bool has_ref, bool calc_ssim)
    {
        destroy();                 // a stream may switch parameter sets
        rs.create(from.H, from.W, to.H, to.W, to.bit_depth);
        hip_ok(hipMalloc(&out, to.frame_bytes()), "hipMalloc");
        hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_out), to.frame_bytes(), hipHostMallocDefault), "hipHostMalloc");
        if (has_ref) {
            hip_ok(hipMalloc(&ref, to.frame_bytes()), "hipMalloc");
            hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_ref), to.frame_bytes(), hipHostMallocDefault), "hipHostMalloc");
            hip_ok(hipMalloc(&sse, 3 * sizeof(double)), "hipMalloc");
            hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_sse), 3 * sizeof(double), hipHostMallocDefault), "hipHostMalloc");
            sse_ws_bytes = std::max(dcvc_sse_workspace_bytes(1, to.H, to.W), dcvc_sse_workspace_bytes(2, to.H / 2, to.W / 2));
            hip_ok(hipMalloc(&sse_ws, static_cast<size_t>(sse_ws_bytes)), "hipMalloc");
        }
        if (calc_ssim) {
            hip_ok(hipMalloc(&ssim, 3 * sizeof(double)), "hipMalloc");
            hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_ssim), 3 * sizeof(double), hipHostMallocDefault), "hipHostMalloc");
            ssim_ws_bytes = std::max(dcvc_msssim_workspace_bytes(1, to.H, to.W), dcvc_msssim_workspace_bytes(2, to.H / 2, to.W / 2));
            hip_ok(hipMalloc(&ssim_ws, static_cast<size_t>(ssim_ws_bytes)), "hipMalloc");
        }
    }
    void destroy()
    {
        if (rs.plan_y) rs.destroy();
        for (void* d : {static_cast<void*>(out), static_cast<void*>(ref), static_cast<void*>(sse), static_cast<void*>(ssim), sse_ws,
                        ssim_ws}) {
            if (d) hip_ok(hipFree(d), "hipFree");
        }
        for (void* h : {static_cast<void*>(h_out), static_cast<void*>(h_ref), static_cast<void*>(h_sse), static_cast<void*>(h_ssim)}) {
            if (h) hip_ok(hipHostFree(h), "hipHostFree");
        }
        *this = ScaledOut{};
    }
};

// --interpolate N[:R[:LAMBDA[:LIMIT]]] / --interp-log FILE / --interp-ref FILE (decode) and --frame-step N (encode):
// what the flags alone decide is refused before a model is loaded
struct InterpArgs {
    bool on = false;
    int n = 2, range = 7, lambda = 4, limit = 8;       // the defaults are untuned
    std::string log, ref;
};

InterpArgs interp_args(const Args& a, bool encoding)
{
    InterpArgs p;
    if (encoding) {
        for (const char* k : {"interpolate", "interp-log", "interp-ref"}) {
            if (a.has(k)) die(std::string("--") + k + " is a decoder flag: encode codes every N-th picture with --frame-step N");
        }
        return p;
    }
    if (a.has("frame-step")) die("--frame-step is an encoder flag: decode shows N times the pictures with --interpolate N");
    if (!a.has("interpolate")) {
        for (const char* k : {"interp-log", "interp-ref"}) {
            if (a.has(k)) die(std::string("--") + k + " needs --interpolate");
        }
        return p;
    }
    if (a.has("interp-ref") && !a.has("interp-log")) die("--interp-ref needs --interp-log: the PSNRs of the in-between pictures go there");
    const std::string s = a.str("interpolate");
    std::vector<std::string> parts;
    for (size_t at = 0;;) {
        const size_t c = s.find(':', at);
        parts.push_back(s.substr(at, c == std::string::npos ? c : c - at));
        if (c == std::string::npos) break;
        at = c + 1;
    }
    const unsigned long long hi[4] = {8, 15, 255, 255};
    unsigned long long v[4] = {2, 7, 4, 8};
    bool ok = parts.size() <= 4;
    for (size_t i = 0; ok && i < parts.size(); ++i) ok = parse_uint(parts[i], hi[i], v[i]);
    if (!ok || v[0] < 2) {
        die("--interpolate must be N[:R[:LAMBDA[:LIMIT]]] with integers in 2..8, 0..15, 0..255 and 0..255, got " + s);
    }
    p.n = static_cast<int>(v[0]); p.range = static_cast<int>(v[1]); p.lambda = static_cast<int>(v[2]); p.limit = static_cast<int>(v[3]);
    const std::string t = a.str("src-type", "yuv420");
    if (t != "yuv420" && t != "yuv422" && t != "yuv444") die("--interpolate is for planar YUV pictures: --src-type " + t + " pictures are not interpolated yet");
    p.log = a.str("interp-log");
    if (a.has("interp-log") && (p.log.empty() || is_dash(p.log))) die("--interp-log needs a file name (not -: a log goes to a file of its own)");
    p.ref = a.str("interp-ref");
    if (a.has("interp-ref") && (p.ref.empty() || is_dash(p.ref))) die("--interp-ref needs a file name (not -)");
    p.on = true;
    return p;
}

int frame_step_arg(const Args& a)
{
    if (!a.has("frame-step")) return 1;
    const int n = int_arg(a, "frame-step", 1, 2, 8);
    if (a.has("deinterlace")) die("--frame-step and --deinterlace: a field's neighbour in time would be dropped; decimate the deinterlaced clip");
    if (a.has("ivtc")) die("--frame-step and --ivtc: the pulldown cycle would be broken; decimate the restored clip");
    const std::string t = a.str("src-type", "yuv420");
    if (t == "png" || t == "png16") die("--frame-step reads raw and Y4M sources: --src-type " + t + " is a directory of PNG pictures");
    return n;
}

// decode --interpolate: N - 1 pictures between every two decoded pictures of one size. The state is a device copy of the previous
// output picture as the metrics see it (behind --out-size, before grain and pad). begin() searches the arriving picture's luma
// against it once; between() makes the picture of phase k: the selection, Y in one interpolation call, U and V in another; keep()
// takes the arriving picture as the next pair's first.
struct Interpolator {
    InterpArgs arg;
    Geometry g;                    // the pictures arriving
    bool active = false, have_prev = false;
    uint8_t* prev = nullptr;
    uint8_t* mid = nullptr;
    int16_t* d_mv = nullptr;
    int16_t* d_plan = nullptr;
    uint8_t* d_wb = nullptr;
    uint32_t* d_sad = nullptr;     // --interp-log: the winners' SADs
    // the counters of fallen blocks, one per in-between picture, read back when all have been used and at the end: the summary
    // line counts the repeated pictures without a wait per picture
    static constexpr int kRing = 1024;
    uint32_t* d_fall = nullptr;
    int ring_n = 0;
    void* d_ws = nullptr;
    long long ws_bytes = 0;
    uint32_t* h_sad = nullptr;     // pinned, --interp-log
    int bh = 0, bw = 0;
    long long out_idx = 0, decoded = 0, between_n = 0, repeated = 0;
    std::string records;
    // --interp-ref
    PictureFile ref_file;
    uint8_t* h_ref = nullptr;      // pinned
    uint8_t* d_ref = nullptr;
    double* d_sse = nullptr;
    double* h_sse = nullptr;       // pinned
    void* sse_ws = nullptr;
    long long sse_ws_bytes = 0;
    void create(const InterpArgs& p, const Geometry& og, const std::string& in_format)
    {
        // a stream may switch parameter sets: the stage restarts (the caller has flushed the counters), the counts and the log go on
        release();
        arg = p;
        g = og;
        active = true;
        have_prev = false;
        if (og.rgb || og.wire >= 0 || (og.pix() && og.pix_fmt != DCVC_PIX_YUV422P && og.pix_fmt != DCVC_PIX_YUV444P)) {
            die("--interpolate is for planar YUV pictures: these pictures are not interpolated yet");
        }
        bh = (g.H + 15) / 16; bw = (g.W + 15) / 16;
        const size_t nb = static_cast<size_t>(bh) * bw;
        ws_bytes = dcvc_motion_search_workspace_bytes(g.H, g.W);
        if (ws_bytes <= 0) die("--interpolate: the output size is outside the search's limits");
        hip_ok(hipMalloc(&prev, g.frame_bytes()), "hipMalloc");
        hip_ok(hipMalloc(&mid, g.frame_bytes()), "hipMalloc");
        hip_ok(hipMalloc(&d_mv, nb * 2 * sizeof(int16_t)), "hipMalloc");
        hip_ok(hipMalloc(&d_plan, nb * 4 * sizeof(int16_t)), "hipMalloc");
        hip_ok(hipMalloc(&d_wb, nb), "hipMalloc");
        hip_ok(hipMalloc(&d_sad, nb * sizeof(uint32_t)), "hipMalloc");
        hip_ok(hipMalloc(&d_fall, kRing * sizeof(uint32_t)), "hipMalloc");
        hip_ok(hipMalloc(&d_ws, static_cast<size_t>(ws_bytes)), "hipMalloc");
        if (!arg.log.empty()) hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_sad), (nb + 1) * sizeof(uint32_t), hipHostMallocDefault), "hipHostMalloc");
        if (!arg.ref.empty()) {
            if (ref_file.fd < 0) ref_file.open(arg.ref, in_format);
            if (ref_file.y4m) {
                const dcvc_y4m_info& i = ref_file.info;
                const int fmt = g.pix() ? g.pix_fmt : DCVC_PIX_YUV420P;
                if (i.width != g.W || i.height != g.H || i.bit_depth != g.bit_depth || i.pix_fmt != fmt) {
                    die("--interp-ref: " + ref_file.path + " holds " + std::to_string(i.width) + "x" + std::to_string(i.height) + " pictures of " +
                        std::to_string(i.bit_depth) + " bits, the output is " + std::to_string(g.W) + "x" + std::to_string(g.H) + " " + chroma_name(g) +
                        " of " + std::to_string(g.bit_depth) + " bits");
                }
            }
            hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_ref), g.frame_bytes(), hipHostMallocDefault), "hipHostMalloc");
            hip_ok(hipMalloc(&d_ref, g.frame_bytes()), "hipMalloc");
            hip_ok(hipMalloc(&d_sse, 3 * sizeof(double)), "hipMalloc");
            hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_sse), 3 * sizeof(double), hipHostMallocDefault), "hipHostMalloc");
            sse_ws_bytes = std::max(dcvc_sse_workspace_bytes(1, g.H, g.W), dcvc_sse_workspace_bytes(2, g.Hc(), g.Wc()));
            hip_ok(hipMalloc(&sse_ws, static_cast<size_t>(sse_ws_bytes)), "hipMalloc");
        }
    }
    // cur: the picture arriving (planes Y, U, V back to back). false: it is the first of its size, nothing lies in front of it
    bool begin(const uint8_t* cur, hipStream_t st)
    {
        if (!have_prev) return false;
        const int dt = g.hbd() ? DCVC_SAMPLE_U16 : DCVC_SAMPLE_U8;
        abi_ok(dcvc_motion_search(cur, g.W, prev, g.W, dt, g.bit_depth, g.H, g.W, arg.range, arg.lambda, d_mv, bh, bw, nullptr, nullptr, d_ws,
                                  ws_bytes, st), "motion search");
        return true;
    }
    // the picture at k / N between the previous picture and cur; it stays valid until the next call
    const uint8_t* between(const uint8_t* cur, int k, hipStream_t st)
    {
        const int es = g.hbd() ? 2 : 1, dt = g.hbd() ? DCVC_SAMPLE_U16 : DCVC_SAMPLE_U8;
        const long long ny = static_cast<long long>(g.H) * g.W, nc = static_cast<long long>(g.Hc()) * g.Wc();
        const int sx = g.Wc() != g.W ? 1 : 0, sy = g.Hc() != g.H ? 1 : 0;
        const size_t nb = static_cast<size_t>(bh) * bw;
        if (ring_n == kRing) flush(st);
        uint32_t* d_fallen = d_fall + ring_n;
        hip_ok(hipMemsetAsync(d_fallen, 0, sizeof(uint32_t), st), "hipMemset");
        abi_ok(dcvc_interp_select(prev, g.W, cur, g.W, dt, g.bit_depth, g.H, g.W, d_mv, bh, bw, k, arg.n, arg.limit, d_plan, d_wb, bh, bw,
                                  h_sad ? d_sad : nullptr, d_fallen, st), "interp select");
        abi_ok(dcvc_interp_planes(prev, g.W, ny, cur, g.W, ny, mid, g.W, ny, dt, g.H, g.W, 1, 0, 0, d_plan, d_wb, bh, bw, k, arg.n, d_fallen,
                                  bh * bw, st), "interp (Y)");
        abi_ok(dcvc_interp_planes(prev + ny * es, g.Wc(), nc, cur + ny * es, g.Wc(), nc, mid + ny * es, g.Wc(), nc, dt, g.Hc(), g.Wc(), 2, sx, sy,
                                  d_plan, d_wb, bh, bw, k, arg.n, d_fallen, bh * bw, st), "interp (U, V)");
        ++between_n;
        if (h_sad) log_picture(k, d_fallen, st);
        ++ring_n;
        ++out_idx;
        return mid;
    }
    // the counters used so far -> repeated
    void flush(hipStream_t st)
    {
        std::vector<uint32_t> f(static_cast<size_t>(ring_n));
        if (ring_n > 0) {
            hip_ok(hipMemcpyAsync(f.data(), d_fall, f.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H");
            hip_ok(hipStreamSynchronize(st), "sync");
        }
        for (uint32_t v : f) repeated += 2ULL * v > static_cast<unsigned long long>(bh) * bw;
        ring_n = 0;
    }
    // one output picture of --interp-ref: an in-between picture is measured against it, a decoded picture's entry is dropped
    bool next_ref()
    {
        if (h_ref == nullptr) return false;
        if (!ref_file.read(h_ref, g.frame_bytes())) die("--interp-ref: " + ref_file.path + " is shorter than the output");
        return true;
    }
    // --interp-log: one small copy and one wait per in-between picture
    void log_picture(int k, const uint32_t* d_fallen, hipStream_t st)
    {
        const size_t nb = static_cast<size_t>(bh) * bw;
        const int es = g.hbd() ? 2 : 1, dt = g.hbd() ? DCVC_SAMPLE_U16 : DCVC_SAMPLE_U8;
        const size_t ny = g.y_bytes(), nc = static_cast<size_t>(g.Hc()) * g.Wc();
        hip_ok(hipMemcpyAsync(h_sad, d_sad, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H");
        hip_ok(hipMemcpyAsync(h_sad + nb, d_fallen, sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H");
        const bool measured = next_ref();
        if (measured) {
            hip_ok(hipMemcpyAsync(d_ref, h_ref, g.frame_bytes(), hipMemcpyHostToDevice, st), "H2D");
            abi_ok(dcvc_sse_ws(d_ref, dt, mid, dt, 1, g.H, g.W, g.W, static_cast<long long>(ny), d_sse, sse_ws, sse_ws_bytes, st), "sse (Y)");
            abi_ok(dcvc_sse_ws(d_ref + ny * es, dt, mid + ny * es, dt, 2, g.Hc(), g.Wc(), g.Wc(), static_cast<long long>(nc), d_sse + 1, sse_ws,
                               sse_ws_bytes, st), "sse (U, V)");
            hip_ok(hipMemcpyAsync(h_sse, d_sse, 3 * sizeof(double), hipMemcpyDeviceToHost, st), "D2H");
        }
        hip_ok(hipStreamSynchronize(st), "sync");
        unsigned long long ssad = 0;
        for (size_t b = 0; b < nb; ++b) ssad += h_sad[b];
        const unsigned long long fallen = h_sad[nb];
        const bool rep = 2 * fallen > nb;
        records += std::string(records.empty() ? "" : ",") + "\n    {\"out_idx\": " + std::to_string(out_idx) + ", \"after\": " + std::to_string(decoded - 1) +
                   ", \"k\": " + std::to_string(k) + ", \"blocks\": " + std::to_string(nb) + ", \"fallen\": " + std::to_string(fallen) +
                   ", \"repeated\": " + std::to_string(rep ? 1 : 0) + ", \"sum_sad\": " + std::to_string(ssad);
        if (measured) {
            const double peak = static_cast<double>((1 << g.bit_depth) - 1);
            records += ", \"psnr_y\": " + jnum(psnr_of_sse(h_sse[0], static_cast<double>(ny), peak)) + ", \"psnr_u\": " +
                       jnum(psnr_of_sse(h_sse[1], static_cast<double>(nc), peak)) + ", \"psnr_v\": " + jnum(psnr_of_sse(h_sse[2], static_cast<double>(nc), peak));
        }
        records += "}";
    }
    // cur becomes the previous picture; it was output picture out_idx
    void keep(const uint8_t* cur, hipStream_t st)
    {
        hip_ok(hipMemcpyAsync(prev, cur, g.frame_bytes(), hipMemcpyDeviceToDevice, st), "D2D");
        have_prev = true;
        ++decoded;
        ++out_idx;
        next_ref();
    }
    // the summary line's tail and --interp-log's file
    std::string finish(hipStream_t st)
    {
        if (!arg.on) return "";
        if (active) flush(st);
        if (!arg.log.empty()) {
            const std::string text = "{\n  \"n\": " + std::to_string(arg.n) + ",\n  \"range\": " + std::to_string(arg.range) + ",\n  \"lambda\": " +
                                     std::to_string(arg.lambda) + ",\n  \"limit\": " + std::to_string(arg.limit) + ",\n  \"block\": 16,\n  \"width\": " +
                                     std::to_string(g.W) + ",\n  \"height\": " + std::to_string(g.H) + ",\n  \"pictures\": [" + records +
                                     (records.empty() ? "" : "\n  ") + "]\n}\n";
            FILE* lf = fopen(arg.log.c_str(), "wb");
            if (!lf || fwrite(text.data(), 1, text.size(), lf) != text.size() || fclose(lf) != 0) die("cannot write " + arg.log);
        }
        return ", interpolate x" + std::to_string(arg.n) + " (" + std::to_string(between_n) + " in-between pictures, " + std::to_string(repeated) +
               " repeated)";
    }
    void release()
    {
        for (void* p : {static_cast<void*>(prev), static_cast<void*>(mid), static_cast<void*>(d_mv), static_cast<void*>(d_plan), static_cast<void*>(d_wb),
                        static_cast<void*>(d_sad), static_cast<void*>(d_fall), d_ws, static_cast<void*>(d_ref), static_cast<void*>(d_sse), sse_ws}) {
            if (p) hip_ok(hipFree(p), "hipFree");
        }
        for (void* h : {static_cast<void*>(h_sad), static_cast<void*>(h_ref), static_cast<void*>(h_sse)}) {
            if (h) hip_ok(hipHostFree(h), "hipHostFree");
        }
        prev = mid = d_wb = d_ref = h_ref = nullptr;
        d_mv = d_plan = nullptr;
        d_sad = d_fall = h_sad = nullptr;
        d_ws = sse_ws = nullptr;
        d_sse = h_sse = nullptr;
    }
    void destroy()
    {
        release();
        ref_file.close();
    }
};

// ------------------------------------------------------------------------------------ picture hashes
// --hash-log / --verify-hash: CRC-32 of every output picture's bytes in raw file layout, hashed on the device
// (dcvc_crc32_segments, one segment per plane); only the CRC words travel to the host.
struct HashPicture {
    uint32_t crc = 0;
    std::vector<uint32_t> planes;
};

struct HashManifest {
    std::string src_type;
    int depth = 0, W = 0, H = 0;
    std::vector<HashPicture> pictures;
    uint32_t sequence = 0;
    long long total_bytes = 0;
};

std::string hex8(uint32_t v)
{
    char buf[16];
    snprintf(buf, sizeof(buf), "%08x", v);
    return buf;
}

// # dcvc-hash 1 crc32 <src_type> <bit_depth> <width> <height> / <idx> <crc> <plane crc> ... / sequence <crc> <total bytes>
std::string manifest_text(const HashManifest& m)
{
    std::string s = "# dcvc-hash 1 crc32 " + m.src_type + " " + std::to_string(m.depth) + " " + std::to_string(m.W) + " " +
                    std::to_string(m.H) + "\n";
    for (size_t i = 0; i < m.pictures.size(); ++i) {
        s += std::to_string(i) + " " + hex8(m.pictures[i].crc);
        for (uint32_t p : m.pictures[i].planes) s += " " + hex8(p);
        s += "\n";
    }
    return s + "sequence " + hex8(m.sequence) + " " + std::to_string(m.total_bytes) + "\n";
}

// the structure of a manifest, strictly; whether its CRCs are the run's is --verify-hash's business
HashManifest read_manifest(const std::string& path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) die("--verify-hash: cannot open " + path);
    const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    auto bad = [&](const std::string& why) { die("--verify-hash: " + path + " is no hash manifest: " + why); };
    if (text.empty() || text.back() != '\n') bad("the last line is not terminated");
    std::vector<std::vector<std::string>> lines;
    for (size_t at = 0; at < text.size();) {
        const size_t nl = text.find('\n', at);
        std::vector<std::string> tok;
        for (size_t t = at; t <= nl;) {
            const size_t sp = std::min(text.find(' ', t), nl);
            tok.push_back(text.substr(t, sp - t));
            t = sp + 1;
        }
        lines.push_back(tok);
        at = nl + 1;
    }
    auto dec = [&](const std::string& s, long long& v) {
        if (s.empty() || s.size() > 18 || s.find_first_not_of("0123456789") != std::string::npos || (s.size() > 1 && s[0] == '0')) return false;
        v = atoll(s.c_str());
        return true;
    };
    auto hex = [&](const std::string& s, uint32_t& v) {
        if (s.size() != 8 || s.find_first_not_of("0123456789abcdef") != std::string::npos) return false;
        v = static_cast<uint32_t>(strtoul(s.c_str(), nullptr, 16));
        return true;
    };
    HashManifest m;
    const std::vector<std::string>& h = lines[0];
    if (h.size() != 8 || h[0] != "#" || h[1] != "dcvc-hash") bad("no '# dcvc-hash 1 crc32 <src_type> <bit_depth> <width> <height>' header");
    if (h[2] != "1") bad("version " + h[2] + " (this tool reads version 1)");
    if (h[3] != "crc32") bad("algorithm " + h[3] + " (this tool hashes with crc32)");
    long long v[3];
    for (int i = 0; i < 3; ++i) {
        if (!dec(h[5 + static_cast<size_t>(i)], v[i]) || v[i] < 1 || v[i] > (1 << 20)) bad("bad numbers in the header");
    }
    m.src_type = h[4];
    m.depth = static_cast<int>(v[0]); m.W = static_cast<int>(v[1]); m.H = static_cast<int>(v[2]);
    // one segment: the packed pixels (RGB; uyvy, yuy2, v210); two: Y and the interleaved chroma
    const bool packed = is_rgb_name(m.src_type) || m.src_type == "uyvy" || m.src_type == "yuy2" || m.src_type == "v210";
    const bool semi = m.src_type == "nv12" || m.src_type == "nv21" || m.src_type == "nv16";
    const size_t planes = packed ? 1 : semi ? 2 : 3;
    if (!packed && !semi && m.src_type != "yuv420" && m.src_type != "yuv422" && m.src_type != "yuv444") {
        bad("unknown source type " + m.src_type);
    }
    if (lines.size() < 2 || lines.back()[0] != "sequence") bad("no sequence line at the end");
    for (size_t i = 1; i + 1 < lines.size(); ++i) {
        const std::vector<std::string>& t = lines[i];
        const std::string what = "line " + std::to_string(i + 1);
        HashPicture p;
        p.planes.resize(planes);
        if (t.size() != 2 + planes || t[0] != std::to_string(i - 1) || !hex(t[1], p.crc)) bad(what + ": no '<idx> <crc> <plane crc> ...' of picture " + std::to_string(i - 1));
        for (size_t k = 0; k < planes; ++k) {
            if (!hex(t[2 + k], p.planes[k])) bad(what + ": a CRC is 8 lowercase hex digits");
        }
        m.pictures.push_back(p);
    }
    const std::vector<std::string>& s = lines.back();
    if (s.size() != 3 || !hex(s[1], m.sequence) || !dec(s[2], m.total_bytes)) bad("no 'sequence <crc> <total bytes>' line at the end");
    return m;
}

// the hashed segments of one picture in file layout: its planes
int hash_segments(const Geometry& g, long long* off, long long* len)
{
    if (g.rgb) {
        off[0] = 0; len[0] = static_cast<long long>(g.frame_bytes());
        return 1;
    }
    const long long es = g.hbd() ? 2 : 1, y = static_cast<long long>(g.y_bytes()) * es, uv = static_cast<long long>(g.uv_bytes()) * es;
    if (g.wire >= 0) {
        // the wire picture: Y and the interleaved chroma (nv21, nv16), or the whole picture (uyvy, yuy2, v210)
        const long long total = static_cast<long long>(g.file_bytes());
        const bool semi = g.wire == DCVC_WIRE_NV21 || g.wire == DCVC_WIRE_NV16;
        off[0] = 0; len[0] = semi ? y : total;
        if (!semi) return 1;
        off[1] = y; len[1] = total - y;
        return 2;
    }
    off[0] = 0; len[0] = y;
    if (g.pix_fmt == DCVC_PIX_NV12) {
        off[1] = y; len[1] = uv;
        return 2;
    }
    off[1] = y; len[1] = uv / 2;
    off[2] = y + uv / 2; len[2] = uv / 2;
    return 3;
}

// what the flags alone decide is refused before a model is loaded; --verify-hash's file is read there too
struct HashRun {
    std::string log, verify;
    HashManifest expect, got;
    uint32_t* d_crc = nullptr;
    uint32_t* h_crc = nullptr;     // pinned
    bool on() const { return !log.empty() || !verify.empty(); }
    void parse(const Args& a, bool encoding)
    {
        if (a.has("verify-hash") && encoding) die("--verify-hash is a decoder flag: encode writes a manifest with --hash-log, decode checks it");
        if (a.has("hash-log") && encoding && a.has("inter") && a.num("intra-period", -1) != 1) {
            die("--hash-log on encode is for all-intra runs (no --inter, or --intra-period 1): the inter encoders reconstruct no "
                "pictures; hash the decoder's output instead");
        }
        log = a.str("hash-log");
        verify = a.str("verify-hash");
        if (a.has("hash-log") && log.empty()) die("--hash-log needs a file name");
        if (a.has("verify-hash") && verify.empty()) die("--verify-hash needs a file name");
        if (!verify.empty()) expect = read_manifest(verify);
    }
    // the run's source type and bit depth, known before the first picture
    void begin(const char* type, int depth)
    {
        if (!on()) return;
        got.src_type = type; got.depth = depth;
        if (!verify.empty() && (expect.src_type != got.src_type || expect.depth != depth)) {
            die("--verify-hash: " + verify + " holds " + expect.src_type + " pictures of " + std::to_string(expect.depth) + " bits, this run's are " +
                got.src_type + " of " + std::to_string(depth) + " bits");
        }
        hip_ok(hipMalloc(&d_crc, 16 * sizeof(uint32_t)), "hipMalloc");
        hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_crc), 16 * sizeof(uint32_t), hipHostMallocDefault), "hipHostMalloc");
    }
    // the output pictures' size, known before the first of them is decoded
    void size(int W, int H)
    {
        if (!on()) return;
        if (got.W != 0 && (got.W != W || got.H != H)) {
            die("picture hashes: the stream switches from " + std::to_string(got.W) + "x" + std::to_string(got.H) + " to " + std::to_string(W) +
                "x" + std::to_string(H) + ", a manifest holds pictures of one size");
        }
        got.W = W; got.H = H;
        if (!verify.empty() && (expect.W != W || expect.H != H)) {
            die("--verify-hash: " + verify + " holds " + std::to_string(expect.W) + "x" + std::to_string(expect.H) + " pictures, this run's are " +
                std::to_string(W) + "x" + std::to_string(H));
        }
    }
    [[noreturn]] void mismatch(const std::string& what) const
    {
        fprintf(stderr, "dcvc: --verify-hash: %s\n", what.c_str());
        exit(3);
    }
    // one output picture on the device (g.file_bytes() bytes in file layout); waits for the stream
    void picture(const uint8_t* dev, const Geometry& g, hipStream_t st)
    {
        long long off[3], len[3];
        const int n = hash_segments(g, off, len);
        abi_ok(dcvc_crc32_segments(dev, off, len, n, d_crc, st), "crc32");
        hip_ok(hipMemcpyAsync(h_crc, d_crc, static_cast<size_t>(n) * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H");
        hip_ok(hipStreamSynchronize(st), "sync");
        HashPicture p;
        for (int k = 0; k < n; ++k) {
            p.planes.push_back(h_crc[k]);
            p.crc = dcvc_crc32_combine(p.crc, h_crc[k], len[k]);
        }
        const size_t idx = got.pictures.size();
        if (!verify.empty()) {
            if (idx >= expect.pictures.size()) {
                mismatch("picture " + std::to_string(idx) + " was decoded, " + verify + " holds " + std::to_string(expect.pictures.size()) + " pictures");
            }
            const HashPicture& e = expect.pictures[idx];
            const char* names = n == 1 ? "P" : "YUV";      // P: the packed pixels; nv12, nv21, nv16: Y and the interleaved chroma
            for (int k = 0; k < n; ++k) {
                if (e.planes[static_cast<size_t>(k)] != p.planes[static_cast<size_t>(k)]) {
                    mismatch("picture " + std::to_string(idx) + ", plane " + std::to_string(k) + " (" + (n == 2 && k == 1 ? "UV" : std::string(1, names[k])) +
                             "): expected " + hex8(e.planes[static_cast<size_t>(k)]) + ", got " + hex8(p.planes[static_cast<size_t>(k)]));
                }
            }
            if (e.crc != p.crc) mismatch("picture " + std::to_string(idx) + ", whole picture: expected " + hex8(e.crc) + ", got " + hex8(p.crc));
        }
        got.sequence = dcvc_crc32_combine(got.sequence, p.crc, static_cast<long long>(g.file_bytes()));
        got.total_bytes += static_cast<long long>(g.file_bytes());
        got.pictures.push_back(p);
    }
    void finish()
    {
        if (!on()) return;
        if (d_crc) hip_ok(hipFree(d_crc), "hipFree");
        if (h_crc) hip_ok(hipHostFree(h_crc), "hipHostFree");
        d_crc = h_crc = nullptr;
        if (!log.empty()) {
            const std::string text = manifest_text(got);
            FILE* lf = fopen(log.c_str(), "wb");
            if (!lf || fwrite(text.data(), 1, text.size(), lf) != text.size()) die("cannot write " + log);
            fclose(lf);
        }
        if (!verify.empty()) {
            if (expect.pictures.size() != got.pictures.size()) {
                mismatch(std::to_string(got.pictures.size()) + " pictures were decoded, " + verify + " holds " + std::to_string(expect.pictures.size()));
            }
            if (expect.sequence != got.sequence || expect.total_bytes != got.total_bytes) {
                mismatch("sequence: expected " + hex8(expect.sequence) + " over " + std::to_string(expect.total_bytes) + " bytes, got " +
                         hex8(got.sequence) + " over " + std::to_string(got.total_bytes));
            }
            fprintf(g_msg, "verified %zu pictures against %s: sequence %s\n", got.pictures.size(), verify.c_str(), hex8(got.sequence).c_str());
        }
    }
};

// x_hat (fp16 [rows][g.Wp][3], top-left H x W) -> the distortion planes in b.y16 and the output samples in file layout in
// b.out8 (RGB, the other chroma formats and high bit depths: only when `samples`; 8-bit YUV420 always writes them)
void x_hat_to_picture(const Geometry& g, const DeviceBuffers& b, const char* xh, bool samples)
{
    char* y16 = static_cast<char*>(b.y16);
    if (g.rgb16()) {
        // fp32 [3][H][W] (the distortion planes) in y16, the writer's packed u16 pixels in out8
        abi_ok(dcvc_x_to_rgb16_cs(xh, g.Wp, g.H, g.W, g.bit_depth, y16, samples ? b.out8 : nullptr, g.matrix, g.range, g.yuv_depth, b.st),
               "x_to_rgb16_cs");
    } else if (g.rgb) {
        // rgb16 [3][H][W] fp16 (the distortion planes) in y16, the writer's packed u8 pixels in out8
        abi_ok(dcvc_x_to_rgb_cs(xh, g.Wp, g.H, g.W, y16, samples ? b.out8 : nullptr, g.matrix, g.range, g.yuv_depth, b.st), "x_to_rgb_cs");
    } else if (g.pix() || g.hbd()) {
        // fp32 distortion planes [H][W] + [2][Hc][Wc] in y16, the output samples in file layout in out8
        abi_ok(dcvc_x_to_pix(xh, g.Wp, g.H, g.W, g.yuv_fmt(), g.bit_depth, y16, samples ? b.out8 : nullptr, b.st), "x_to_pix");
    } else {
        // 8-bit YUV420: fp16 distortion planes, which the decode log sums on the host
        abi_ok(dcvc_x_to_yuv420(xh, g.Wp, g.H, g.W, y16, y16 + g.y_bytes() * 2, b.out8, b.out8 + g.y_bytes(), b.st), "x_to_yuv420");
    }
}

// --quality-log / --target-psnr: the encoder's own measurement of a reconstruction against the source samples
// it uploaded, with the calls and the geometry decode --ref uses for the source type and depth; every sum stays on the device.
// 8-bit YUV420, where the decoder sums fp16 planes on the host: dcvc_x_to_pix(DCVC_PIX_YUV420P, 8) -> dcvc_sse_ws, fp32 planes
// that hold the same values.
struct PictureQuality {
    double psnr = 0, y = 0, u = 0, v = 0;
};

struct QualityMeter {
    uint8_t* src = nullptr;        // per slot: the source picture as planar samples (RGB: u8 or u16 [3][H][W]; YUV: Y, Cb, Cr planes)
    void* dist = nullptr;          // the reconstruction's distortion planes: fp16 (8-bit RGB) or fp32 [3][H][W], fp32 [H][W] + [2][Hc][Wc] (YUV)
    double* sse = nullptr;
    double* h_sse = nullptr;       // pinned
    void* ws = nullptr;
    long long ws_bytes = 0;
    void create(const Geometry& g, int slots)
    {
        hip_ok(hipMalloc(&src, g.frame_bytes() * static_cast<size_t>(slots)), "hipMalloc");
        hip_ok(hipMalloc(&dist, g.rgb16() ? g.y_bytes() * 12 : g.rgb ? g.y_bytes() * 6 : (g.y_bytes() + g.uv_bytes()) * 4), "hipMalloc");
        hip_ok(hipMalloc(&sse, 3 * sizeof(double)), "hipMalloc");
        hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_sse), 3 * sizeof(double), hipHostMallocDefault), "hipHostMalloc");
        ws_bytes = g.rgb ? dcvc_sse_workspace_bytes(3, g.H, g.W)
                         : std::max(dcvc_sse_workspace_bytes(1, g.H, g.W), dcvc_sse_workspace_bytes(2, g.Hc(), g.Wc()));
        hip_ok(hipMalloc(&ws, static_cast<size_t>(ws_bytes)), "hipMalloc");
    }
    // the picture in the staging planes b.yuv8 (at the coded size: behind --scale's resampler) -> slot; in stream order
    void capture(const Geometry& g, const DeviceBuffers& b, int slot)
    {
        uint8_t* dst = src + g.frame_bytes() * static_cast<size_t>(slot);
        if (g.rgb16()) {
            abi_ok(dcvc_rgb16_to_x_cs(b.yuv8, 3LL * g.W, 3, 1, g.bit_depth, g.H, g.W, nullptr, 3, dst, g.matrix, g.range, g.yuv_depth, b.st),
                   "rgb16_to_x_cs (planar source)");
        } else if (g.rgb) {
            abi_ok(dcvc_rgb_to_x_cs(b.yuv8, 3LL * g.W, 3, 1, g.H, g.W, nullptr, 3, dst, g.matrix, g.range, g.yuv_depth, b.st),
                   "rgb_to_x_cs (planar source)");
        } else if (g.pix()) {
            abi_ok(dcvc_pix_to_x(b.yuv8, g.pix_fmt, g.bit_depth, g.H, g.W, nullptr, 3, dst, b.st), "pix_to_x (planar source)");
        } else {
            hip_ok(hipMemcpyAsync(dst, b.yuv8, g.frame_bytes(), hipMemcpyDeviceToDevice, b.st), "D2D");
        }
    }
    // x_hat (fp16 [rows][g.Wp][3]) against the source in `slot`; waits for the stream
    PictureQuality measure(const Geometry& g, const char* xh, int slot, hipStream_t st)
    {
        const uint8_t* s = src + g.frame_bytes() * static_cast<size_t>(slot);
        PictureQuality q;
        if (g.rgb16()) {
            const size_t plane = g.y_bytes();
            abi_ok(dcvc_x_to_rgb16_cs(xh, g.Wp, g.H, g.W, g.bit_depth, dist, nullptr, g.matrix, g.range, g.yuv_depth, st), "x_to_rgb16_cs");
            abi_ok(dcvc_sse_ws(s, DCVC_SAMPLE_U16, dist, DCVC_SAMPLE_F32, 3, g.H, g.W, g.W, static_cast<long long>(plane), sse, ws, ws_bytes, st),
                   "sse");
            hip_ok(hipMemcpyAsync(h_sse, sse, 3 * sizeof(double), hipMemcpyDeviceToHost, st), "D2H");
            hip_ok(hipStreamSynchronize(st), "sync");
            q.psnr = psnr_of_sse((h_sse[0] + h_sse[1]) + h_sse[2], 3.0 * static_cast<double>(plane), static_cast<double>((1 << g.bit_depth) - 1));
            return q;
        }
        if (g.rgb) {
            const size_t plane = g.y_bytes();
            abi_ok(dcvc_x_to_rgb_cs(xh, g.Wp, g.H, g.W, dist, nullptr, g.matrix, g.range, g.yuv_depth, st), "x_to_rgb_cs");
            abi_ok(dcvc_sse_ws(s, DCVC_SAMPLE_U8, dist, DCVC_SAMPLE_F16, 3, g.H, g.W, g.W, static_cast<long long>(plane), sse, ws, ws_bytes, st),
                   "sse");
            hip_ok(hipMemcpyAsync(h_sse, sse, 3 * sizeof(double), hipMemcpyDeviceToHost, st), "D2H");
            hip_ok(hipStreamSynchronize(st), "sync");
            q.psnr = psnr_of_sse((h_sse[0] + h_sse[1]) + h_sse[2], 3.0 * static_cast<double>(plane));
            return q;
        }
        const size_t ny = g.y_bytes(), nc = static_cast<size_t>(g.Hc()) * g.Wc(), es = g.hbd() ? 2 : 1;
        const int dt = g.hbd() ? DCVC_SAMPLE_U16 : DCVC_SAMPLE_U8;
        const double peak = static_cast<double>((1 << g.bit_depth) - 1);
        abi_ok(dcvc_x_to_pix(xh, g.Wp, g.H, g.W, g.yuv_fmt(), g.bit_depth, dist, nullptr, st), "x_to_pix");
        const char* dist_uv = static_cast<const char*>(dist) + ny * 4;
        abi_ok(dcvc_sse_ws(s, dt, dist, DCVC_SAMPLE_F32, 1, g.H, g.W, g.W, static_cast<long long>(ny), sse, ws, ws_bytes, st), "sse (Y)");
        abi_ok(dcvc_sse_ws(s + ny * es, dt, dist_uv, DCVC_SAMPLE_F32, 2, g.Hc(), g.Wc(), g.Wc(), static_cast<long long>(nc), sse + 1, ws,
                           ws_bytes, st), "sse (U, V)");
        hip_ok(hipMemcpyAsync(h_sse, sse, 3 * sizeof(double), hipMemcpyDeviceToHost, st), "D2H");
        hip_ok(hipStreamSynchronize(st), "sync");
        q.y = psnr_of_sse(h_sse[0], static_cast<double>(ny), peak);
        q.u = psnr_of_sse(h_sse[1], static_cast<double>(nc), peak);
        q.v = psnr_of_sse(h_sse[2], static_cast<double>(nc), peak);
        q.psnr = (6 * q.y + q.u + q.v) / 8;
        return q;
    }
    void destroy()
    {
        for (void* d : {static_cast<void*>(src), dist, static_cast<void*>(sse), ws}) {
            if (d) hip_ok(hipFree(d), "hipFree");
        }
        if (h_sse) hip_ok(hipHostFree(h_sse), "hipHostFree");
        *this = QualityMeter{};
    }
};

// one coded unit in --quality-log
struct QualityUnit {
    bool intra = false;
    int first_picture = 0, qp = 0, trials = 0;
    long long bytes = 0;
    double psnr = 0;
    std::vector<PictureQuality> pictures;
};

// dcvc_rc_pick_qp_for_quality's callback: the trial coding of a unit at qp -> its quality
struct QualityTrial {
    std::function<double(int)> run;
    static double call(int qp, void* user) { return static_cast<QualityTrial*>(user)->run(qp); }
};

// one source picture in --scene-log
struct ScenePicture {
    long long sad = 0;
    double mafd = 0, score = 0;
    bool detected = false, intra = false;
    const char* reason = nullptr;      // "first", "period", "cut"
};

// one coded unit in --rc-log
struct RateUnit {
    bool intra = false;
    int qp = 0, probes = 0;
    long long predicted_bytes = -1, bytes = 0;      // -1: no prediction (the feedback loop does not probe)
};

// --read-ahead N: one reader thread fills a ring of N + 1 pinned host slots with the source's pictures while the
// main thread codes. The main thread allocates and frees the slots and makes every HIP call; the thread only reads
// (PictureFile::next) and hands slots over under a mutex and a condition variable. A slot goes back to the thread once the
// upload that read it has completed.
struct ReadAhead {
    struct Slot {
        uint8_t* p = nullptr;      // pinned
        bool full = false;
        PictureFile::Status status = PictureFile::End;
        double read_ms = 0;        // when the picture was complete in host memory, since the run started
    };
    std::vector<Slot> slots;
    size_t head = 0, tail = 0;     // the next slot the coder takes, the next the reader fills
    std::mutex m;
    std::condition_variable cv;
    bool stop = false;
    std::thread th;
    // at most `limit` pictures of `bytes` bytes are read; the first slot that is no picture (the end, a broken source) is the last
    void start(PictureFile& f, size_t bytes, int n_slots, int limit, std::chrono::steady_clock::time_point t0)
    {
        slots.resize(static_cast<size_t>(n_slots));
        for (Slot& s : slots) hip_ok(hipHostMalloc(reinterpret_cast<void**>(&s.p), bytes, hipHostMallocDefault), "hipHostMalloc");
        th = std::thread([this, &f, bytes, limit, t0] {
            for (int k = 0; k < limit; ++k) {
                Slot* s = nullptr;
                {
                    std::unique_lock<std::mutex> lk(m);
                    cv.wait(lk, [&] { return stop || !slots[tail].full; });
                    if (stop) return;
                    s = &slots[tail];
                }
                const PictureFile::Status status = f.next(s->p, bytes);
                const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                {
                    std::lock_guard<std::mutex> lk(m);
                    s->status = status; s->read_ms = ms; s->full = true;
                    tail = (tail + 1) % slots.size();
                }
                cv.notify_all();
                if (status != PictureFile::Picture) return;
            }
        });
    }
    // the next slot in reading order, once it is full; it stays the coder's until release()
    Slot& take()
    {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return slots[head].full; });
        return slots[head];
    }
    void release()
    {
        {
            std::lock_guard<std::mutex> lk(m);
            slots[head].full = false;
            head = (head + 1) % slots.size();
        }
        cv.notify_all();
    }
    void finish()
    {
        {
            std::lock_guard<std::mutex> lk(m);
            stop = true;
        }
        cv.notify_all();
        if (th.joinable()) th.join();
        for (Slot& s : slots) hip_ok(hipHostFree(s.p), "hipHostFree");
        slots.clear();
    }
};

// one coded unit in --latency-log
struct LatencyUnit {
    bool intra = false;
    int first_picture = 0, pictures = 0, qp = 0;
    long long bytes = 0;                  // a parameter set written in front of the unit included
    double read_ms = 0, out_ms = 0;
};

// the source frames a run reads from a regular file of file_total pictures: encode's own arithmetic below (-n counts coded
// pictures; --deinterlace field codes two a frame; --ivtc film reads whole cycles of 5 for 4), for --crop auto, which spreads
// its probes over them before the loop is set up
long long source_frames_of(long long file_total, bool has_n, long long n, bool two_fields, bool film)
{
    long long total = two_fields ? std::min<long long>(2 * file_total, 1 << 30) : file_total;
    if (film) total = 4 * (total / 5) + total % 5;
    const long long frame_num = has_n ? std::min(n, total) : total;
    if (frame_num <= 0) return 0;
    return two_fields ? (frame_num + 1) / 2 : film ? std::min(file_total, 5 * ((frame_num + 3) / 4)) : frame_num;
}

// ------------------------------------------------------------------------------------ encode
int encode(const Args& a)
{
    const int batch = batch_arg(a);
    const SceneArgs scene = scene_args(a, batch);
    const QualityArgs quality = quality_args(a, batch);
    const RateArgs rate = rate_args(a, batch);
    const ColourArgs colour = colour_args(a);
    HashRun hash;
    hash.parse(a, true);
    const PipeArgs pipe = pipe_args(a, true);
    const VbvArgs vbv_arg = vbv_args(a, batch, true);
    if (is_dash(a.str("o"))) g_msg = stderr;      // stdout carries the stream
    if (batch > 1 && a.has("inter") && a.num("intra-period", -1) != 1) {
        die("--batch codes intra pictures only: all-intra runs (no --inter, or --intra-period 1)");
    }
    SrcType type = src_type(a.str("src-type", "yuv420"));
    int depth = bit_depth_arg(a, type);
    const SizeArg scale = size_arg(a, "scale");
    const int wire = wire_arg(a, true);
    rgb16_arg(a, true);
    const DenoiseArgs denoise = denoise_args(a, true);
    const GrainArgs grain = grain_args(a, true);
    IvtcArgs ivtc = ivtc_args(a, true);
    DeinterlaceArgs deint = deinterlace_args(a, true);
    const CropArgs crop = crop_args(a, true);
    interp_args(a, true);
    int pic_w = a.num("W", 0), pic_h = a.num("H", 0);
    // -i *.y4m: the header supplies the size, the source type and the bit depth; flags that disagree are refused
    PictureFile src_file;
    src_file.step = frame_step_arg(a);         // --frame-step: the reader's clip is the decimated one, in front of every stage
    if (pipe.in_is_y4m(a.str("i"))) {
        src_file.open(a.str("i"), pipe.in_format, deint.on || ivtc.on);
        const Y4mSource y = y4m_source(src_file, a, true);
        // an It / Ib file supplies the field order; without --deinterlace or --ivtc it was refused above
        if (src_file.interlacing != 0) {
            const bool bff = src_file.interlacing == 2;
            if (a.has("field-order") && (deint.on ? deint.bff : ivtc.bff) != bff) {
                die(src_file.path + " is " + (bff ? "bottom" : "top") + " field first (I" + (bff ? "b" : "t") + "), not --field-order " +
                    a.str("field-order"));
            }
            deint.bff = ivtc.bff = bff;
        }
        type = y.type; depth = y.depth;
        pic_w = src_file.info.width; pic_h = src_file.info.height;
        if (scale.on && pix_fmt_of(type) >= 0) {
            die(std::string("--scale is for --src-type yuv420: ") + src_type_name(type) + " sources are not resampled yet");
        }
    }
    const bool rgb = is_rgb(type);
    PngDir pngs;
    if (is_png(type)) {
        // the size of the first picture; -W / -H, when given, must agree with it
        pngs = png_dir(a.str("i"));
        if (type == SrcType::Png16) png16_info(pngs.path(1), pic_w, pic_h);
        else abi_ok(dcvc_png_info(pngs.path(1).c_str(), &pic_w, &pic_h), "png info");
        if ((a.has("W") && a.num("W", 0) != pic_w) || (a.has("H") && a.num("H", 0) != pic_h)) {
            die(pngs.path(1) + " is " + std::to_string(pic_w) + "x" + std::to_string(pic_h) + ", not the -W x -H given");
        }
    } else if (rgb && (!a.has("W") || !a.has("H"))) {
        die(std::string("--src-type ") + src_type_name(type) + " needs -W and -H");
    }
    // gf: the file's pictures, which the reader and the upload see; gs: the source's pictures, which everything else derives from
    // (--crop: the window's); g: the pictures that are coded (--scale: another size, resampled on the device)
    const Geometry gf = geometry(pic_h, pic_w, rgb, depth, pix_fmt_of(type), wire);
    CropStage cs;
    if (crop.on) {
        // the window is settled before a model is loaded: a manual one is checked, auto probes the clip
        cs.create(crop, gf, deint.on || ivtc.on);
        if (crop.automatic) {
            if (src_file.fd < 0) src_file.open(a.str("i"), pipe.in_format);
            if (!src_file.regular) die("--crop auto needs a seekable source; give --crop WxH+X+Y");
            const long long probe_frames = source_frames_of(src_file.count(gf.file_bytes()), a.has("n"), a.num("n", 0), deint.on && deint.field,
                                                            ivtc.on && ivtc.film);
            if (probe_frames <= 0) die("no pictures to code");
            cs.detect(src_file, gf, probe_frames);
        }
        fprintf(g_msg, "crop: %s, %dx%d+%d+%d of %dx%d (%d of %zu pictures voted)\n", cs.arg.mode(), cs.arg.w, cs.arg.h, cs.arg.x, cs.arg.y, gf.W,
                gf.H, cs.votes, cs.probes.size());
        cs.write_log(gf, wire >= 0 ? wire_name(wire) : src_type_name(type));
    }
    Geometry gs = cs.active ? geometry(cs.arg.h, cs.arg.w, rgb, depth, pix_fmt_of(type), wire) : gf;
    if (cs.active && wire >= 0) gs.file_bytes();      // a window the wire format has no picture of is refused here
    if (rgb) colour.apply(gs);
    if (scale.on) check_ratio("--scale", gs.W, gs.H, scale.W, scale.H);
    const Geometry g = scale.on ? geometry(scale.H, scale.W, false, depth) : gs;
    if (deint.on && gs.Hc() < 2) die("--deinterlace needs planes of at least 2 rows");
    if (ivtc.on && gs.Hc() < 2) die("--ivtc needs planes of at least 2 rows");
    // --vbv-maxrate / --vbv-bufsize: the decoder-buffer model counts the pixels of the coded size, as the rate controller does
    dcvc_rc_vbv* vbv = nullptr;
    if (vbv_arg.on) {
        vbv = dcvc_rc_vbv_create(vbv_arg.maxrate, vbv_arg.bufsize, vbv_arg.init, static_cast<long long>(g.H) * g.W);
        if (!vbv) die(std::string("--vbv-maxrate / --vbv-bufsize: ") + dcvc_last_error());
    }
    if (scene.on) {
        const int kind = weight_kind(a.str("inter"));      // from the file's header, before either model is built
        if (kind == 2 || kind == 3) {
            die("--scene-cut needs a one-picture inter model (LD): " + a.str("inter") + " codes chunks of 8 pictures, a P unit "
                "always holds 8 and the container has no picture count, so a chunk cannot be cut short at a scene change");
        }
    }
    Codecs c = make_codecs(a.str("intra"), a.str("inter"));
    const bool force_intra = !c.has_inter();
    const int intra_period = force_intra ? 1 : a.num("intra-period", -1);
    const int reset_interval = a.num("reset-interval", 32);
    const int qp_i = a.num("qp-i", 32), qp_p = a.num("qp-p", qp_i);
    const int delay = c.frames_per_p;
    if (intra_period > 1 && intra_period % delay != 0) die("intra period must be a multiple of the chunk size");
    long long total = 0;
    if (is_png(type)) {
        total = pngs.count();
    } else {
        if (src_file.fd < 0) src_file.open(a.str("i"), pipe.in_format);
        // a pipe's length is unknown: the loop below learns the clip's end from the reader, -n still caps it
        total = src_file.regular ? src_file.count(gf.file_bytes()) : (1 << 30);
    }
    const bool piped_in = !is_png(type) && !src_file.regular;
    // --deinterlace field: two coded pictures a source frame; -n counts coded pictures, the reader source frames
    const bool two_fields = deint.on && deint.field;
    if (two_fields) total = std::min<long long>(2 * total, 1 << 30);
    // --ivtc film: a complete cycle of 5 source frames gives 4 coded pictures, a ragged last one all of its frames; -n counts coded
    // pictures, the reader source frames
    const long long file_frames = total;
    if (ivtc.on && ivtc.film) total = 4 * (total / IvtcStage::kCycle) + total % IvtcStage::kCycle;
    // pictures to code; from a pipe: an upper bound until the input ends
    int frame_num = a.has("n") ? std::min<long long>(a.num("n", 0), total) : static_cast<int>(total);
    if (frame_num <= 0) die("no pictures to code");
    // ... film: whole cycles are read until they hold the pictures wanted
    const int source_frames = two_fields ? (frame_num + 1) / 2
                              : ivtc.on && ivtc.film ? static_cast<int>(std::min<long long>(file_frames, IvtcStage::kCycle * ((frame_num + 3LL) / 4)))
                                                     : frame_num;
    const int read_ahead = pipe.read_ahead >= 0 ? pipe.read_ahead : piped_in ? 2 : 0;    DeviceBuffers b = make_buffers(g, std::max(delay, batch), false, scene.on);
    // --quality-log / --target-psnr: every converted picture's source samples stay on the device, one slot per picture of a unit
    QualityMeter meter;
    if (quality.on()) meter.create(g, std::max(delay, batch));
    std::vector<QualityUnit> quality_units;
    void* trial_state = nullptr;           // --target-psnr, --vbv-*: the inter codec's state in front of a P unit's trials / codings
    long long trial_state_bytes = 0;
    void* kept_dev = nullptr;              // ... and what the last trial that met left: the intra x_hat, or the inter codec's state
    size_t kept_cap = 0;
    // --hash-log: the intra encoder's reconstruction as the decoder would write it, with the source's type and depth at the
    // coded size
    // a wire format's source pictures are unpacked into b.yuv8, where the carrier type's upload lands, and the hashed
    // reconstruction is packed: everything between the two is the carrier type's run
    WireStage ws;
    ws.create(g);
    hash.begin(wire >= 0 ? wire_name(wire) : src_type_name(type), depth);
    hash.size(g.W, g.H);
    auto hash_x_hat = [&](const char* xh) {
        x_hat_to_picture(g, b, xh, true);
        if (wire >= 0) ws.pack(g, b.out8, b.st);
        hash.picture(wire >= 0 ? ws.out : b.out8, g, b.st);
    };
    // --scale: the source picture's own staging, pinned and on the device, in front of b.yuv8
    Resampler rs;
    uint8_t* h_full = nullptr;
    uint8_t* d_full = nullptr;
    if (scale.on) {
        rs.create(gs.H, gs.W, g.H, g.W, depth);
        hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h_full), gs.frame_bytes(), hipHostMallocDefault), "hipHostMalloc");
        hip_ok(hipMalloc(&d_full, gs.frame_bytes()), "hipMalloc");
    }
    // --denoise: the uploads, the resampler and the unpack fill `staging`; the filter's output buffer takes b.yuv8's place, so
    // the conversion, the quality meter and the padding pictures of a ragged chunk read the filtered picture where it lies
    uint8_t* const staging = b.yuv8;
    Denoiser dn;
    if (denoise.on) dn.create(g, denoise);
    GrainMeter gm;
    if (grain.log_on) {
        gm.create(g, grain, denoise.spatial, denoise.temporal);
        dn.meter = &gm;
    }
    // --deinterlace: the upload and the unpack fill one of the filter's two input buffers at the source size; it writes where
    // they would have: the resampler's input with --scale, `staging` without
    Deinterlacer di;
    if (deint.on) di.create(gs, deint);
    // --ivtc sits where the deinterlacer does
    IvtcStage iv;
    if (ivtc.on) iv.create(gs, ivtc);
    const int pad_b = g.Hp - g.H, pad_r = g.Wp - g.W;
    std::vector<uint8_t> out, payload;
    dcvc::stream::SpsTable sps;
    // -o on a pipe ("-", a FIFO), or --flush-units 1: every parameter set and unit is written as soon as it is complete, and `out`
    // holds one unit at a time; a regular file without the flag is written once at the end
    const std::string out_name = a.str("o");
    const bool streaming = names_a_pipe(out_name) || pipe.flush_units;
    int out_fd = -1;
    if (streaming) {
        out_fd = is_dash(out_name) ? 1 : ::open(out_name.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (out_fd < 0) die("cannot write " + out_name);
    }
    long long out_bytes = 0;               // bytes handed to out_fd
    std::vector<LatencyUnit> latency;
    const auto t0 = std::chrono::steady_clock::now();
    auto now_ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    // --read-ahead: the source's pictures arrive in the ring's pinned slots instead of the one pinned buffer of each path
    ReadAhead ra;
    if (read_ahead > 0) ra.start(src_file, gf.file_bytes(), read_ahead + 1, source_frames, t0);
    bool slot_held = false;                // a slot whose upload is in flight: released behind convert()'s synchronisation
    double last_read_ms = 0;               // when the last source picture was complete in host memory
    std::string input_error;               // a pipe that broke off inside a picture: the run ends as at the end of the input, with status 2
    bool input_done = false;               // a pipe has ended: what was read is the clip
    auto source_ended = [&](PictureFile::Status st) {
        if (!piped_in) die(st == PictureFile::Broken ? src_file.error : "short read");
        input_done = true;
        if (st == PictureFile::Broken) {
            input_error = src_file.error;
        } else if (src_file.partial > 0) {
            fprintf(stderr, "dcvc: warning: %s ends with %zu bytes that are no whole picture (%zu bytes each): dropped\n",
                    src_file.path.c_str(), src_file.partial, gf.file_bytes());
        }
    };
    // the next picture of -i in pinned memory - `own`, or a read-ahead slot; nullptr when a pipe has ended
    auto next_source = [&](uint8_t* own) -> const uint8_t* {
        if (read_ahead > 0) {
            ReadAhead::Slot& s = ra.take();
            if (s.status != PictureFile::Picture) {
                source_ended(s.status);
                return nullptr;
            }
            slot_held = true;
            last_read_ms = s.read_ms;
            return s.p;
        }
        const PictureFile::Status st = src_file.next(own, gf.file_bytes());
        if (st != PictureFile::Picture) {
            source_ended(st);
            return nullptr;
        }
        last_read_ms = now_ms();
        return own;
    };
    if (cs.active) cs.allocate(gf);
    if (crop.on) cs.open_out(gs);
    // the pinned buffer a source picture is read into when no read-ahead slot holds it
    uint8_t* const h_own = cs.active ? cs.h_in : scale.on ? h_full : wire >= 0 ? ws.h_in : b.h_yuv;
    // the source picture in pinned memory at h -> its planes at dst on the device: the upload, a wire format's unpack, and with
    // --crop the window (the upload then lands in the stage's buffer of the file's size)
    auto upload = [&](uint8_t* dst, const uint8_t* h) {
        if (cs.active) cs.upload(gf, gs, dst, h, b.st);
        else if (wire >= 0) ws.upload(gs, dst, b.st, h);
        else hip_ok(hipMemcpyAsync(dst, h, gs.frame_bytes(), hipMemcpyHostToDevice, b.st), "H2D");
        if (crop.on) cs.written(gs, dst, b.st);
    };
    // the next source picture -> the device's staging planes; convert() turns them into fp16 x at dst (pixel stride ldx).
    // false: the input has ended (a pipe; a regular file was counted)
    auto load_picture = [&]() -> bool {
        if (is_png(type)) {
            if (!pngs.read(b.h_yuv, g)) die("short read");
            last_read_ms = now_ms();
            hip_ok(hipMemcpyAsync(b.yuv8, b.h_yuv, g.frame_bytes(), hipMemcpyHostToDevice, b.st), "H2D");
            return true;
        }
        if (ivtc.on) {
            // a cycle of source frames is read and measured when no frame waits; every upload is waited for (the words are needed
            // on the host), so the pinned memory it read is free again at once
            if (!iv.pending()) {
                int got = 0;
                while (got < iv.cycle() && iv.frames() < source_frames && !input_done) {
                    const uint8_t* h = next_source(h_own);
                    if (h == nullptr) break;
                    upload(iv.next_input(), h);
                    iv.measure(gs, b.st);
                    if (slot_held) ra.release();
                    slot_held = false;
                    ++got;
                }
                iv.close_cycle(got);
                if (!iv.pending()) return false;
            }
            iv.serve(gs, scale.on ? d_full : staging, b.st);
            if (scale.on) rs.run(d_full, staging, b.st);
            if (denoise.on) b.yuv8 = dn.run(g, staging, b.st);
            return true;
        }
        // --deinterlace field: the second picture of a frame comes from the frame on the device
        const bool fresh = !deint.on || di.wants_frame();
        const uint8_t* h = fresh ? next_source(h_own) : nullptr;
        if (fresh && h == nullptr) return false;
        if (deint.on) {
            if (fresh) upload(di.next_input(), h);
            di.run(gs, scale.on ? d_full : staging, b.st);
            if (scale.on) rs.run(d_full, staging, b.st);
        } else if (scale.on) {
            upload(d_full, h);
            rs.run(d_full, staging, b.st);
        } else {
            upload(staging, h);
        }
        // once per source picture, in source order: recodes and padding pictures come from what this left
        if (denoise.on) b.yuv8 = dn.run(g, staging, b.st);
        return true;
    };
    // measure (--scene-cut): the picture's luma and its SAD against the previous one ride on the same synchronisation
    int luma_turn = 0;
    auto convert = [&](char* dst, int ldx, bool measure = false, bool has_prev = false) {
        if (g.rgb16()) {
            abi_ok(dcvc_rgb16_to_x_cs(b.yuv8, 3LL * g.W, 3, 1, g.bit_depth, g.H, g.W, dst, ldx, nullptr, g.matrix, g.range, g.yuv_depth, b.st),
                   "rgb16_to_x_cs");
        } else if (rgb) {
            abi_ok(dcvc_rgb_to_x_cs(b.yuv8, 3LL * g.W, 3, 1, g.H, g.W, dst, ldx, nullptr, g.matrix, g.range, g.yuv_depth, b.st), "rgb_to_x_cs");
        } else {
            abi_ok(dcvc_pix_to_x(b.yuv8, g.yuv_fmt(), g.bit_depth, g.H, g.W, dst, ldx, nullptr, b.st), "pix_to_x");
        }
        if (measure) {
            abi_ok(dcvc_luma_sad(dst, ldx, g.H, g.W, has_prev ? b.luma8[luma_turn ^ 1] : nullptr, b.luma8[luma_turn], b.sad, b.st),
                   "luma_sad");
            hip_ok(hipMemcpyAsync(b.h_sad, b.sad, sizeof(unsigned long long), hipMemcpyDeviceToHost, b.st), "D2H");
            luma_turn ^= 1;
        }
        hip_ok(hipStreamSynchronize(b.st), "sync");      // the staging buffers are reused
        if (slot_held) ra.release();                     // ... and so is the read-ahead slot the upload read
        slot_held = false;
    };
    // the unit of `pictures` source pictures from first_picture on, the last of them read at read_ms
    // -> the bytes the unit added to the stream, a parameter set in front of it included
    auto put_unit = [&](bool intra, int qp, int ec, int reset, const std::vector<uint8_t>& pl, int first_picture, int pictures, double read_ms) {
        const size_t before = out.size();
        bool is_new = false;
        const int sps_id = sps.id_for(g.H, g.W, is_new);
        if (is_new) dcvc::stream::put_sps(out, sps_id, g.H, g.W);
        dcvc::stream::put_ip(out, intra, sps_id, qp, ec, reset != 0, pl.data(), pl.size());
        LatencyUnit lu;
        lu.intra = intra; lu.first_picture = first_picture; lu.pictures = pictures; lu.qp = qp; lu.read_ms = read_ms;
        lu.bytes = static_cast<long long>(out.size() - before);
        if (streaming) {
            // write() hands the bytes to the OS: nothing of them stays in a buffer of the tool's
            if (!write_all(out_fd, out.data(), out.size())) {
                if (errno == EPIPE) output_closed(out_name);
                die("cannot write " + out_name);
            }
            out_bytes += static_cast<long long>(out.size());
            out.clear();
            lu.out_ms = now_ms();
        }
        if (!pipe.latency_log.empty()) latency.push_back(lu);
        return lu.bytes;
    };
    // --target-bpp: all-intra runs search the q_index of every picture on the size probe, runs with an inter model follow the
    // feedback controller (rate_control.code_sequence with TargetBpp)
    const bool rate_search = rate.on && intra_period == 1;
    const double pixels = static_cast<double>(g.H) * g.W;
    // ... or, with --rc-mode probe, search every P unit's q_index on the inter model's probe (rate_control.code_sequence_probed)
    const bool rate_probe = rate.on && !rate_search && rate.probe;
    int start_q = qp_i, pictures_coded = 0;
    int quality_start_i = qp_i, quality_start_p = qp_i;      // --target-psnr: the previous unit's q_index, per type
    dcvc_rc* ctl = nullptr;
    if (rate.on && !rate_search && !rate_probe) {
        ctl = dcvc_rc_create(rate.target_bpp, pixels, qp_i, rate.horizon, rate.intra_bonus, rate.qp_min, rate.qp_max, 0.049);
        if (!ctl) die(std::string("rate control: ") + dcvc_last_error());
    }
    std::vector<RateUnit> rate_units;
    long long spent_bits = 0;
    std::vector<VbvUnit> vbv_units;
    bool vbv_first_unit = true;            // the first unit has the parameter set in front (one coded size per run)
    struct Probe {
        dcvc_dmci* codec; const void* x; int H, W, pad_b, pad_r; void* st;
        std::map<int, long long> bytes;                // predicted stream bytes of every q_index probed
    };
    // --vbv-*: qp_mode of a unit whose search ran on min(the mode's own budget, the buffer's payload budget) - the largest probed
    // q_index whose prediction fits the own budget (rate_control.vbv_searched_qp_mode): the mode's answer when the cap does not
    // bind, a lower bound of it when it does
    auto searched_qp_mode = [](int qp, const std::map<int, long long>& probed, int64_t own_budget) {
        int best = qp;
        for (const auto& kv : probed) {
            if (8 * kv.second <= own_budget && kv.first > best) best = kv.first;
        }
        return best;
    };
    auto probe_bits = [](int qp, void* user) -> int64_t {
        Probe& p = *static_cast<Probe*>(user);
        int64_t units[2];
        if (dcvc_dmci_estimate_bits(p.codec, p.x, p.H, p.W, qp, p.pad_b, p.pad_r, units, p.st) < 0) return -1;
        const int64_t kept = dcvc_dmci_estimate_symbols(p.codec, 0);
        if (kept < 0) return -1;
        const long long bytes = dcvc_predicted_stream_bytes(units[0], units[1], dcvc_ec_parallel_for(kept));
        if (bytes < 0) return -1;
        p.bytes[qp] = bytes;
        return 8 * bytes;
    };
    struct InterProbe {
        dcvc_dmcld* ld; dcvc_dmcht* ht; const void* x; int H, W, pad_b, pad_r; void* st;
        std::map<int, long long> bytes;
    };
    auto inter_probe_bits = [](int qp, void* user) -> int64_t {
        InterProbe& p = *static_cast<InterProbe*>(user);
        int64_t units[2];
        const int rc = p.ld ? dcvc_dmcld_estimate_bits(p.ld, p.x, p.H, p.W, qp, p.pad_b, p.pad_r, units, p.st)
                            : dcvc_dmcht_estimate_bits(p.ht, p.x, p.H, p.W, qp, p.pad_b, p.pad_r, units, p.st);
        if (rc < 0) return -1;
        const int64_t kept = p.ld ? dcvc_dmcld_estimate_symbols(p.ld) : dcvc_dmcht_estimate_symbols(p.ht);
        if (kept < 0) return -1;
        const long long bytes = dcvc_predicted_stream_bytes(units[0], units[1], dcvc_ec_parallel_for(kept));
        if (bytes < 0) return -1;
        p.bytes[qp] = bytes;
        return 8 * bytes;
    };
    // --scene-cut: every picture is converted and measured before its type is known (one-picture units: I and P share
    // the x layout, ldx == 3); the detector may turn a scheduled P picture into an I picture, never the other way
    dcvc_scd* scd = nullptr;
    std::vector<ScenePicture> scene_pictures;
    if (scene.on) {
        scd = dcvc_scd_create(scene.threshold, scene.min_gap, static_cast<long long>(g.H) * g.W);
        if (!scd) die(std::string("scene cut: ") + dcvc_last_error());
    }
    int idx = 0;
    // (--ivtc: frames of the last cycle may still wait when the pipe has ended)
    while (idx < frame_num && (!input_done || iv.pending())) {
        bool intra = is_intra_picture(idx, intra_period);
        if (scd) {
            if (!load_picture()) break;
            if (quality.on()) meter.capture(g, b, 0);
            convert(static_cast<char*>(b.x), 3, true, idx > 0);
            ScenePicture sp;
            sp.sad = idx > 0 ? static_cast<long long>(*b.h_sad) : 0;
            const int as_intra = dcvc_scd_push(scd, idx, sp.sad, intra ? 1 : 0);
            abi_ok(as_intra, "scene cut");
            int detected = 0;
            abi_ok(dcvc_scd_last(scd, &sp.mafd, &sp.score, &detected), "scene cut");
            sp.detected = detected != 0;
            sp.reason = intra ? (idx == 0 ? "first" : "period") : (as_intra ? "cut" : nullptr);
            intra = as_intra != 0;
            sp.intra = intra;
            scene_pictures.push_back(sp);
        }
        if (intra && batch > 1) {
            // up to `batch` intra pictures in one call, each in its own slot [H][W][3]; the units go out in picture order
            int nb = std::min(batch, frame_num - idx);
            const size_t slot = static_cast<size_t>(g.H) * g.W * 3 * 2, slot_hat = static_cast<size_t>(g.Hp) * g.Wp * 3 * 2;
            double read_ms[16];
            for (int j = 0; j < nb; ++j) {
                char* dst = static_cast<char*>(b.x) + slot * j;
                if (!load_picture()) nb = j;      // a pipe ended: a short last batch
                if (j >= nb) break;
                read_ms[j] = last_read_ms;
                if (quality.on()) meter.capture(g, b, j);
                convert(dst, 3);
            }
            if (nb == 0) break;
            int ecs[16];
            abi_ok(dcvc_dmci_compress_batch(c.intra, nb, b.x, g.H, g.W, qp_i, pad_b, pad_r, b.x_hat, ecs, b.st), "intra compress");
            for (int j = 0; j < nb; ++j) {
                const long long nbytes = dcvc_dmci_get_stream_at(c.intra, j, nullptr, 0);
                abi_ok(nbytes, "get_stream_at");
                payload.resize(static_cast<size_t>(nbytes));
                abi_ok(dcvc_dmci_get_stream_at(c.intra, j, payload.data(), payload.size()), "get_stream_at");
                const char* xh = static_cast<const char*>(b.x_hat) + slot_hat * j;
                if (c.ld) abi_ok(dcvc_dmcld_add_ref_feature_from_frame(c.ld, xh, g.Hp, g.Wp, 1, b.st), "add_ref");
                if (c.ht) abi_ok(dcvc_dmcht_add_ref_feature_from_frame(c.ht, xh, g.Hp, g.Wp, 1, b.st), "add_ref");
                if (hash.on()) hash_x_hat(xh);
                if (quality.on()) {
                    QualityUnit qu;
                    qu.intra = true; qu.first_picture = idx + j; qu.qp = qp_i; qu.bytes = nbytes;
                    qu.pictures.push_back(meter.measure(g, xh, j, b.st));
                    qu.psnr = qu.pictures[0].psnr;
                    quality_units.push_back(qu);
                }
                put_unit(true, qp_i, ecs[j], 0, payload, idx + j, 1, read_ms[j]);
            }
            idx += nb;
            continue;
        }
        int want = intra ? 1 : std::min(delay, frame_num - idx);
        const int slots = intra ? 1 : delay;
        const int ldx = 3 * slots;
        for (int j = 0; j < slots && !scd; ++j) {
            char* dst = static_cast<char*>(b.x) + 6 * j;
            // a short last chunk repeats its final picture (test_video.py:104-110); a pipe that ends inside the chunk makes it one
            if (j < want && !load_picture()) want = j;
            if (want == 0) break;
            if (quality.on() && j < want) meter.capture(g, b, j);
            convert(dst, ldx);
        }
        if (want == 0) break;
        int ec = 0, reset = 0, qp = qp_i;
        long long nbytes = 0;
        RateUnit ru;
        ru.intra = intra;
        // --vbv-*: what the unit may take, and what its payload may (rate_control.vbv_payload_budget): the container's bytes
        // around the longest payload that fits bound those around every shorter one
        VbvUnit vu;
        int64_t vbv_avail = 0, vbv_payload_avail = 0;
        auto vbv_overhead = [&](size_t payload_bytes) {
            return static_cast<long long>(dcvc::stream::unit_overhead(payload_bytes, vbv_first_unit, g.H, g.W));
        };
        if (vbv) {
            vu.fullness_before = dcvc_rc_vbv_fullness(vbv);
            vbv_avail = dcvc_rc_vbv_available(vbv);
            const int64_t longest = std::min<int64_t>(std::max<int64_t>(vbv_avail, 0) / 8, (1 << 30) - 1);
            vbv_payload_avail = vbv_avail - 8 * vbv_overhead(static_cast<size_t>(longest));
        }
        if (rate_search) {
            Probe p{c.intra, b.x, g.H, g.W, pad_b, pad_r, b.st, {}};
            const int64_t own = dcvc_rc_intra_budget_bits(rate.target_bpp, pixels, idx, spent_bits);
            qp = dcvc_rc_pick_qp_for_budget(probe_bits, &p, vbv ? std::min(own, vbv_payload_avail) : own, rate.qp_min, rate.qp_max, &ru.probes);
            abi_ok(qp, "size probe");
            ru.predicted_bytes = p.bytes.at(qp);
            vu.qp_mode = searched_qp_mode(qp, p.bytes, own);
        } else if (ctl) {
            qp = dcvc_rc_next_qp(ctl, intra ? 1 : 0);
            abi_ok(qp, "rate control");
        } else if (rate_probe && intra) {
            qp = std::min(rate.qp_max, std::max(rate.qp_min, start_q + rate.intra_bonus));
        } else if (rate_probe) {
            InterProbe p{c.ld, c.ht, b.x, g.H, g.W, pad_b, pad_r, b.st, {}};
            const int64_t budget = dcvc_rc_unit_budget_bits(rate.target_bpp, pixels, pictures_coded, spent_bits, rate.horizon, want);
            abi_ok(budget, "rate control");
            qp = dcvc_rc_pick_qp_near(inter_probe_bits, &p, vbv ? std::min(budget, vbv_payload_avail) : budget, start_q, rate.qp_min, rate.qp_max,
                                      &ru.probes);
            abi_ok(qp, "size probe");
            ru.predicted_bytes = p.bytes.at(qp);
            vu.qp_mode = searched_qp_mode(qp, p.bytes, budget);
            start_q = qp;
        }
        // --quality-log / --target-psnr: the unit's reconstruction measured on the device. An I picture's is the intra x_hat; a P
        // unit's comes from dcvc_dmc*_reconstruct, which leaves the temporal state as it is. The padding pictures of a ragged
        // last chunk (slots want .. delay - 1) do not count.
        QualityUnit qu;
        qu.intra = intra; qu.first_picture = idx;
        auto code_intra = [&](int q) {
            ec = dcvc_dmci_compress(c.intra, b.x, g.H, g.W, q, pad_b, pad_r, b.x_hat, b.st);
            abi_ok(ec, "intra compress");
            nbytes = dcvc_dmci_get_stream(c.intra, nullptr, 0);
            payload.resize(static_cast<size_t>(nbytes));
            abi_ok(dcvc_dmci_get_stream(c.intra, payload.data(), payload.size()), "get_stream");
        };
        auto code_inter = [&](int q) {
            if (c.ld) {
                ec = dcvc_dmcld_compress(c.ld, b.x, g.H, g.W, q, reset, pad_b, pad_r, b.st);
                abi_ok(ec, "inter compress");
                nbytes = dcvc_dmcld_get_stream(c.ld, nullptr, 0);
                payload.resize(static_cast<size_t>(nbytes));
                abi_ok(dcvc_dmcld_get_stream(c.ld, payload.data(), payload.size()), "get_stream");
            } else {
                ec = dcvc_dmcht_compress(c.ht, b.x, g.H, g.W, q, reset, pad_b, pad_r, b.st);
                abi_ok(ec, "inter compress");
                nbytes = dcvc_dmcht_get_stream(c.ht, nullptr, 0);
                payload.resize(static_cast<size_t>(nbytes));
                abi_ok(dcvc_dmcht_get_stream(c.ht, payload.data(), payload.size()), "get_stream");
            }
        };
        auto measure_unit = [&]() {
            if (!intra) {
                abi_ok(c.ld ? dcvc_dmcld_reconstruct(c.ld, b.x_hat, b.st) : dcvc_dmcht_reconstruct(c.ht, b.x_hat, b.st), "reconstruct");
            }
            qu.pictures.clear();
            double sum = 0;
            for (int j = 0; j < want; ++j) {
                const char* xh = static_cast<const char*>(b.x_hat) + static_cast<size_t>(j) * g.Hp * g.Wp * 3 * 2;
                qu.pictures.push_back(meter.measure(g, xh, j, b.st));
                sum += qu.pictures.back().psnr;
            }
            qu.psnr = sum / want;
            return qu.psnr;
        };
        if (!intra) reset = (reset_interval > 0 && (idx + delay) % reset_interval == 1) ? 1 : 0;
        if (quality.target_on) {
            // rate_control.code_sequence_quality: the smallest q_index in [--qp-min, --qp-max] whose trial coding meets the target,
            // searched from the previous unit's q_index of the same type (--qp-i for the first). A P unit's trials all start from
            // the state exported once in front of them. The unit is the chosen trial - the last trial that met, or the last
            // trial when none did: every trial that meets leaves its stream, its figures and what the encoder goes on from (the
            // intra x_hat; the inter codec's state behind it) in `kept`, and a chosen trial that was not the last one is put
            // back from there. Coding it again from the same state would give the same bytes and costs a compress.
            int& start = intra ? quality_start_i : quality_start_p;
            int last_q = -1;
            bool first = true;
            if (!intra) {
                const long long sb = c.ld ? dcvc_dmcld_export_state(c.ld, nullptr, 0, b.st) : dcvc_dmcht_export_state(c.ht, nullptr, 0, b.st);
                abi_ok(sb, "export_state");
                if (sb != trial_state_bytes) {
                    if (trial_state) hip_ok(hipFree(trial_state), "hipFree");
                    hip_ok(hipMalloc(&trial_state, static_cast<size_t>(sb)), "hipMalloc");
                    trial_state_bytes = sb;
                }
                abi_ok(c.ld ? dcvc_dmcld_export_state(c.ld, trial_state, static_cast<size_t>(sb), b.st)
                            : dcvc_dmcht_export_state(c.ht, trial_state, static_cast<size_t>(sb), b.st), "export_state");
            }
            auto restore = [&]() {
                abi_ok(c.ld ? dcvc_dmcld_import_state(c.ld, trial_state, static_cast<size_t>(trial_state_bytes), g.H, g.W, b.st)
                            : dcvc_dmcht_import_state(c.ht, trial_state, static_cast<size_t>(trial_state_bytes), g.H, g.W, b.st), "import_state");
            };
            const size_t kept_bytes = intra ? static_cast<size_t>(g.Hp) * g.Wp * 3 * 2 : static_cast<size_t>(trial_state_bytes);
            if (kept_bytes > kept_cap) {
                if (kept_dev) hip_ok(hipFree(kept_dev), "hipFree");
                hip_ok(hipMalloc(&kept_dev, kept_bytes), "hipMalloc");
                kept_cap = kept_bytes;
            }
            int kept_q = -1, kept_ec = 0;
            std::vector<uint8_t> kept_payload;
            QualityUnit kept_unit;
            QualityTrial trial;
            trial.run = [&](int q) {
                if (intra) {
                    code_intra(q);
                } else {
                    if (!first) restore();
                    code_inter(q);
                }
                first = false;
                last_q = q;
                const double got = measure_unit();
                if (got >= quality.target) {
                    kept_q = q; kept_ec = ec; kept_payload = payload; kept_unit = qu;
                    if (intra) {
                        hip_ok(hipMemcpyAsync(kept_dev, b.x_hat, kept_bytes, hipMemcpyDeviceToDevice, b.st), "D2D");
                    } else {
                        abi_ok(c.ld ? dcvc_dmcld_export_state(c.ld, kept_dev, kept_bytes, b.st) : dcvc_dmcht_export_state(c.ht, kept_dev, kept_bytes, b.st),
                               "export_state");
                    }
                }
                return got;
            };
            int trials = 0;
            qp = dcvc_rc_pick_qp_for_quality(QualityTrial::call, &trial, quality.target, start, quality.qp_min, quality.qp_max, &trials);
            abi_ok(qp, "quality search");
            if (qp != last_q && qp == kept_q) {
                ec = kept_ec; payload = kept_payload; qu = kept_unit;
                if (intra) {
                    hip_ok(hipMemcpyAsync(b.x_hat, kept_dev, kept_bytes, hipMemcpyDeviceToDevice, b.st), "D2D");
                } else {
                    abi_ok(c.ld ? dcvc_dmcld_import_state(c.ld, kept_dev, kept_bytes, g.H, g.W, b.st)
                                : dcvc_dmcht_import_state(c.ht, kept_dev, kept_bytes, g.H, g.W, b.st), "import_state");
                }
            } else if (qp != last_q) {
                die("quality search: the chosen q_index " + std::to_string(qp) + " is neither the last trial nor the last that met");
            }
            qu.trials = trials;
            start = qp;
            if (intra) {
                if (c.ld) abi_ok(dcvc_dmcld_add_ref_feature_from_frame(c.ld, b.x_hat, g.Hp, g.Wp, 1, b.st), "add_ref");
                if (c.ht) abi_ok(dcvc_dmcht_add_ref_feature_from_frame(c.ht, b.x_hat, g.Hp, g.Wp, 1, b.st), "add_ref");
                if (hash.on()) hash_x_hat(static_cast<const char*>(b.x_hat));
            }
        } else if (vbv) {
            // rate_control.vbv_fit: coded at the mode's q_index and accepted when the unit fits the buffer - one
            // state export per P unit, no probe. On a miss the state goes back, the largest q_index below whose predicted stream
            // fits the payload budget is searched on the size probe (which leaves the state alone) and coded; the coder may
            // exceed the prediction, so the q_index then steps down until the unit fits or the floor is reached.
            if (!intra && !ctl && !rate_probe) qp = qp_p;
            const int floor_q = rate.on ? rate.qp_min : 0;
            if (vu.qp_mode < 0) vu.qp_mode = qp;      // no search under the cap: what the mode gave
            if (!intra) {
                const long long sb = c.ld ? dcvc_dmcld_export_state(c.ld, nullptr, 0, b.st) : dcvc_dmcht_export_state(c.ht, nullptr, 0, b.st);
                abi_ok(sb, "export_state");
                if (sb != trial_state_bytes) {
                    if (trial_state) hip_ok(hipFree(trial_state), "hipFree");
                    hip_ok(hipMalloc(&trial_state, static_cast<size_t>(sb)), "hipMalloc");
                    trial_state_bytes = sb;
                }
                abi_ok(c.ld ? dcvc_dmcld_export_state(c.ld, trial_state, static_cast<size_t>(sb), b.st)
                            : dcvc_dmcht_export_state(c.ht, trial_state, static_cast<size_t>(sb), b.st), "export_state");
            }
            auto restore = [&]() {
                if (intra) return;
                abi_ok(c.ld ? dcvc_dmcld_import_state(c.ld, trial_state, static_cast<size_t>(trial_state_bytes), g.H, g.W, b.st)
                            : dcvc_dmcht_import_state(c.ht, trial_state, static_cast<size_t>(trial_state_bytes), g.H, g.W, b.st), "import_state");
            };
            auto code = [&](int q) {
                if (intra) code_intra(q); else code_inter(q);
            };
            auto conforms = [&]() { return 8 * (static_cast<long long>(payload.size()) + vbv_overhead(payload.size())) <= vbv_avail; };
            code(qp);
            if (!conforms() && qp > floor_q) {
                restore();      // the probes read the temporal state in front of the unit, and leave it alone
                Probe pi{c.intra, b.x, g.H, g.W, pad_b, pad_r, b.st, {}};
                InterProbe pp{c.ld, c.ht, b.x, g.H, g.W, pad_b, pad_r, b.st, {}};
                std::map<int, long long>& predicted = intra ? pi.bytes : pp.bytes;
                int probes = 0;
                qp = intra ? dcvc_rc_pick_qp_near(probe_bits, &pi, vbv_payload_avail, qp - 1, floor_q, qp - 1, &probes)
                           : dcvc_rc_pick_qp_near(inter_probe_bits, &pp, vbv_payload_avail, qp - 1, floor_q, qp - 1, &probes);
                abi_ok(qp, "size probe");
                ru.probes += probes;
                ru.predicted_bytes = predicted.at(qp);
                code(qp);
                ++vu.recodes;
                while (!conforms() && qp > floor_q) {
                    restore();
                    --qp;
                    ru.predicted_bytes = predicted.count(qp) ? predicted.at(qp) : -1;
                    code(qp);
                    ++vu.recodes;
                }
            }
            if (rate_probe && !intra) start_q = qp;
            if (intra) {
                if (c.ld) abi_ok(dcvc_dmcld_add_ref_feature_from_frame(c.ld, b.x_hat, g.Hp, g.Wp, 1, b.st), "add_ref");
                if (c.ht) abi_ok(dcvc_dmcht_add_ref_feature_from_frame(c.ht, b.x_hat, g.Hp, g.Wp, 1, b.st), "add_ref");
                if (hash.on()) hash_x_hat(static_cast<const char*>(b.x_hat));
            }
        } else if (intra) {
            ec = dcvc_dmci_compress(c.intra, b.x, g.H, g.W, qp, pad_b, pad_r, b.x_hat, b.st);
            abi_ok(ec, "intra compress");
            nbytes = dcvc_dmci_get_stream(c.intra, nullptr, 0);
            payload.resize(static_cast<size_t>(nbytes));
            abi_ok(dcvc_dmci_get_stream(c.intra, payload.data(), payload.size()), "get_stream");
            if (c.ld) abi_ok(dcvc_dmcld_add_ref_feature_from_frame(c.ld, b.x_hat, g.Hp, g.Wp, 1, b.st), "add_ref");
            if (c.ht) abi_ok(dcvc_dmcht_add_ref_feature_from_frame(c.ht, b.x_hat, g.Hp, g.Wp, 1, b.st), "add_ref");
            if (hash.on()) hash_x_hat(static_cast<const char*>(b.x_hat));
        } else {
            if (!ctl && !rate_probe) qp = qp_p;
            if (c.ld) {
                ec = dcvc_dmcld_compress(c.ld, b.x, g.H, g.W, qp, reset, pad_b, pad_r, b.st);
                abi_ok(ec, "inter compress");
                nbytes = dcvc_dmcld_get_stream(c.ld, nullptr, 0);
                payload.resize(static_cast<size_t>(nbytes));
                abi_ok(dcvc_dmcld_get_stream(c.ld, payload.data(), payload.size()), "get_stream");
            } else {
                ec = dcvc_dmcht_compress(c.ht, b.x, g.H, g.W, qp, reset, pad_b, pad_r, b.st);
                abi_ok(ec, "inter compress");
                nbytes = dcvc_dmcht_get_stream(c.ht, nullptr, 0);
                payload.resize(static_cast<size_t>(nbytes));
                abi_ok(dcvc_dmcht_get_stream(c.ht, payload.data(), payload.size()), "get_stream");
            }
        }
        if (quality.on()) {
            if (!quality.target_on) measure_unit();
            qu.qp = qp; qu.bytes = static_cast<long long>(payload.size());
            quality_units.push_back(qu);
        }
        const long long unit_bytes = put_unit(intra, qp, ec, reset, payload, idx, want, last_read_ms);
        if (vbv) {
            // the model counts what the unit added to the file; then the mode's own book-keeping, with the final q_index
            if (unit_bytes != static_cast<long long>(payload.size()) + vbv_overhead(payload.size())) die("vbv: the unit's bytes are not the ones counted");
            const int violated = dcvc_rc_vbv_admit(vbv, 8 * unit_bytes, want);
            abi_ok(violated, "vbv");
            vu.intra = intra; vu.first_picture = idx; vu.pictures = want; vu.qp = qp; vu.probes = ru.probes;
            vu.predicted_bytes = ru.predicted_bytes; vu.bytes = unit_bytes; vu.violated = violated != 0;
            vu.underflow_bits = dcvc_rc_vbv_underflow(vbv);
            vu.fullness_after = dcvc_rc_vbv_fullness(vbv);
            if (vu.violated) {
                fprintf(stderr, "dcvc: warning: the unit at picture %d (%lld bits at q_index %d) exceeds the decoder buffer by %lld bits\n", idx,
                        8 * unit_bytes, qp, vu.underflow_bits);
            }
            vbv_units.push_back(vu);
            vbv_first_unit = false;
        }
        if (rate.on) {
            if (ctl) {
                abi_ok(vbv ? dcvc_rc_update_at(ctl, 8.0 * payload.size(), want, intra ? 1 : 0, qp)
                           : dcvc_rc_update(ctl, 8.0 * payload.size(), want, intra ? 1 : 0), "rate control");
            }
            spent_bits += 8LL * static_cast<long long>(payload.size());
            pictures_coded += want;
            ru.qp = qp;
            ru.bytes = static_cast<long long>(payload.size());
            rate_units.push_back(ru);
        }
        idx += want;
    }
    hip_ok(hipStreamSynchronize(b.st), "sync");
    if (read_ahead > 0) ra.finish();
    frame_num = idx;                       // from a pipe: the pictures the input held
    if (frame_num == 0) die(input_error.empty() ? "no pictures to code" : input_error);
    src_file.close();
    ws.destroy();
    if (scale.on) {
        rs.destroy();
        hip_ok(hipHostFree(h_full), "hipHostFree");
        hip_ok(hipFree(d_full), "hipFree");
    }
    if (crop.on) cs.destroy();
    if (deint.on) {
        fprintf(g_msg, "deinterlace: %s, %s, threshold %d, %lld pictures from %lld frames\n", deint.mode(), deint.order(), deint.threshold,
                di.pictures, di.frames);
        di.destroy();
    }
    if (ivtc.on) {
        fprintf(g_msg, "ivtc: %s, %s, cthresh %d, mi %d, threshold %d, %lld pictures from %lld frames (%lld matched to the previous frame, "
                "%lld deinterlaced, %lld dropped)\n", ivtc.mode(), ivtc.order(), ivtc.cthresh, ivtc.mi, ivtc.threshold, iv.pictures, iv.frames(),
                iv.matched_prev, iv.deinterlaced, iv.dropped);
        iv.write_log();
        iv.destroy();
    }
    if (denoise.on) {
        fprintf(g_msg, "denoise: spatial %d, temporal %d, %lld pictures filtered%s\n", denoise.spatial, denoise.temporal, dn.pictures,
                dn.finish_mc(g, b.st).c_str());
        if (grain.log_on) gm.finish(b.st);
        b.yuv8 = staging;
        dn.destroy();
    }
    if (ctl) dcvc_rc_destroy(ctl);
    hash.finish();
    if (scd) {
        dcvc_scd_destroy(scd);
        int cuts = 0;
        for (const ScenePicture& sp : scene_pictures) cuts += sp.reason && std::strcmp(sp.reason, "cut") == 0;
        fprintf(g_msg, "scene cut: threshold %s, min gap %d, %d of %zu pictures coded as I pictures at a cut\n", jnum(scene.threshold).c_str(),
                scene.min_gap, cuts, scene_pictures.size());
        if (!scene.log.empty()) {
            std::string js = "{\"threshold\": " + jnum(scene.threshold) + ", \"min_gap\": " + std::to_string(scene.min_gap) +
                             ", \"width\": " + std::to_string(g.W) + ", \"height\": " + std::to_string(g.H) + ", \"pictures\": [";
            for (size_t i = 0; i < scene_pictures.size(); ++i) {
                const ScenePicture& sp = scene_pictures[i];
                js += std::string(i ? ", " : "") + "{\"idx\": " + std::to_string(i) + ", \"sad\": " + std::to_string(sp.sad) +
                      ", \"mafd\": " + jnum(sp.mafd) + ", \"score\": " + jnum(sp.score) + ", \"detected\": " +
                      (sp.detected ? "true" : "false") + ", \"type\": \"" + (sp.intra ? "I" : "P") + "\", \"reason\": " +
                      (sp.reason ? "\"" + std::string(sp.reason) + "\"" : std::string("null")) + "}";
            }
            js += "]}\n";
            FILE* lf = fopen(scene.log.c_str(), "wb");
            if (!lf || fwrite(js.data(), 1, js.size(), lf) != js.size()) die("cannot write " + scene.log);
            fclose(lf);
        }
    }
    if (rate.on) {
        const double achieved = static_cast<double>(spent_bits) / (static_cast<double>(frame_num) * pixels);
        fprintf(g_msg, "rate control: target %.4f bpp, coded %.4f bpp in %zu units\n", rate.target_bpp, achieved, rate_units.size());
        if (!rate.log.empty()) {
            std::string js = "{\"target_bpp\": " + jnum(rate.target_bpp) + ", \"achieved_bpp\": " + jnum(achieved) +
                             ", \"width\": " + std::to_string(g.W) + ", \"height\": " + std::to_string(g.H) +
                             ", \"pictures\": " + std::to_string(frame_num) + ", \"qp_min\": " + std::to_string(rate.qp_min) +
                             ", \"qp_max\": " + std::to_string(rate.qp_max) + ", \"mode\": \"" +
                             (rate_search || rate_probe ? "probe" : "feedback") + "\", \"units\": [";
            for (size_t i = 0; i < rate_units.size(); ++i) {
                const RateUnit& u = rate_units[i];
                js += std::string(i ? ", " : "") + "{\"type\": \"" + (u.intra ? "I" : "P") + "\", \"qp\": " + std::to_string(u.qp) +
                      ", \"probes\": " + std::to_string(u.probes) + ", \"predicted_bytes\": " +
                      (u.predicted_bytes < 0 ? std::string("null") : std::to_string(u.predicted_bytes)) +
                      ", \"bytes\": " + std::to_string(u.bytes) + "}";
            }
            js += "]}\n";
            FILE* lf = fopen(rate.log.c_str(), "wb");
            if (!lf || fwrite(js.data(), 1, js.size(), lf) != js.size()) die("cannot write " + rate.log);
            fclose(lf);
        }
    }
    if (vbv) {
        double min_fullness = vbv_arg.init * dcvc_rc_vbv_capacity(vbv);
        long long lowered = 0, recodes = 0, violations = 0;
        for (const VbvUnit& u : vbv_units) {
            min_fullness = std::min(min_fullness, u.fullness_after);
            lowered += u.qp < u.qp_mode;
            recodes += u.recodes;
            violations += u.violated;
        }
        fprintf(g_msg, "vbv: capacity %.0f bits, minimum fullness %.0f bits, %lld of %zu units lowered, %lld recodes, %lld violations\n",
                dcvc_rc_vbv_capacity(vbv), min_fullness, lowered, vbv_units.size(), recodes, violations);
        if (!vbv_arg.log.empty()) {
            std::string js = "{\"maxrate_bpp\": " + jnum(vbv_arg.maxrate) + ", \"bufsize_pictures\": " + jnum(vbv_arg.bufsize) + ", \"init\": " +
                             jnum(vbv_arg.init) + ", \"width\": " + std::to_string(g.W) + ", \"height\": " + std::to_string(g.H) +
                             ", \"rate_bits\": " + jnum(dcvc_rc_vbv_rate(vbv)) + ", \"capacity_bits\": " + jnum(dcvc_rc_vbv_capacity(vbv)) +
                             ", \"units\": [";
            for (size_t i = 0; i < vbv_units.size(); ++i) {
                const VbvUnit& u = vbv_units[i];
                js += std::string(i ? ", " : "") + "{\"type\": \"" + (u.intra ? "I" : "P") + "\", \"first_picture\": " + std::to_string(u.first_picture) +
                      ", \"pictures\": " + std::to_string(u.pictures) + ", \"qp_mode\": " + std::to_string(u.qp_mode) + ", \"qp\": " +
                      std::to_string(u.qp) + ", \"probes\": " + std::to_string(u.probes) + ", \"recodes\": " + std::to_string(u.recodes) +
                      ", \"predicted_bytes\": " + (u.predicted_bytes < 0 ? std::string("null") : std::to_string(u.predicted_bytes)) +
                      ", \"bytes\": " + std::to_string(u.bytes) + ", \"fullness_before\": " + jnum(u.fullness_before) +
                      ", \"fullness_after\": " + jnum(u.fullness_after) + ", \"violated\": " + (u.violated ? "true" : "false") +
                      ", \"underflow_bits\": " + std::to_string(u.underflow_bits) + "}";
            }
            js += "], \"min_fullness\": " + jnum(min_fullness) + ", \"lowered\": " + std::to_string(lowered) + ", \"recodes\": " +
                  std::to_string(recodes) + ", \"violations\": " + std::to_string(violations) + "}\n";
            FILE* lf = fopen(vbv_arg.log.c_str(), "wb");
            if (!lf || fwrite(js.data(), 1, js.size(), lf) != js.size()) die("cannot write " + vbv_arg.log);
            fclose(lf);
        }
        dcvc_rc_vbv_destroy(vbv);
    }
    if (trial_state) hip_ok(hipFree(trial_state), "hipFree");
    if (quality.on()) {
        if (kept_dev) hip_ok(hipFree(kept_dev), "hipFree");
        meter.destroy();
        double sum = 0;
        long long count = 0, total_trials = 0;
        for (const QualityUnit& u : quality_units) {
            for (const PictureQuality& q : u.pictures) sum += q.psnr;
            count += static_cast<long long>(u.pictures.size());
            total_trials += u.trials;
        }
        const double ave = count ? sum / static_cast<double>(count) : 0.0;
        if (quality.target_on) {
            fprintf(g_msg, "quality: target %.4f dB, coded %.4f dB in %zu units, %lld trial codings\n", quality.target, ave, quality_units.size(),
                    total_trials);
        }
        if (!quality.log.empty()) {
            std::string js = "{\"target_psnr\": " + (quality.target_on ? jnum(quality.target) : std::string("null")) +
                             ", \"qp_min\": " + std::to_string(quality.qp_min) + ", \"qp_max\": " + std::to_string(quality.qp_max) +
                             ", \"width\": " + std::to_string(g.W) + ", \"height\": " + std::to_string(g.H) + ", \"src_type\": \"" +
                             src_type_name(type) + "\", \"bit_depth\": " + std::to_string(depth) + ", \"units\": [";
            for (size_t i = 0; i < quality_units.size(); ++i) {
                const QualityUnit& u = quality_units[i];
                std::vector<double> all, py, pu, pv;
                for (const PictureQuality& q : u.pictures) {
                    all.push_back(q.psnr); py.push_back(q.y); pu.push_back(q.u); pv.push_back(q.v);
                }
                js += std::string(i ? ", " : "") + "{\"type\": \"" + (u.intra ? "I" : "P") + "\", \"first_picture\": " +
                      std::to_string(u.first_picture) + ", \"pictures\": " + std::to_string(u.pictures.size()) + ", \"qp\": " +
                      std::to_string(u.qp) + ", \"trials\": " + std::to_string(u.trials) + ", \"bytes\": " + std::to_string(u.bytes) +
                      ", \"psnr\": " + jnum(u.psnr) + ", \"frame_psnr\": " + jlist(all);
                if (!rgb) js += ", \"frame_psnr_y\": " + jlist(py) + ", \"frame_psnr_u\": " + jlist(pu) + ", \"frame_psnr_v\": " + jlist(pv);
                js += "}";
            }
            js += "], \"ave_all_frame_psnr\": " + jnum(ave) + ", \"total_trials\": " + std::to_string(total_trials) + "}\n";
            FILE* lf = fopen(quality.log.c_str(), "wb");
            if (!lf || fwrite(js.data(), 1, js.size(), lf) != js.size()) die("cannot write " + quality.log);
            fclose(lf);
        }
    }
    size_t stream_bytes = out.size();
    if (streaming) {
        stream_bytes = static_cast<size_t>(out_bytes);
        if (out_fd != 1 && ::close(out_fd) != 0) die("cannot write " + out_name);
    } else {
        FILE* of = fopen(a.str("o").c_str(), "wb");
        if (!of || fwrite(out.data(), 1, out.size(), of) != out.size()) die("cannot write " + a.str("o"));
        fclose(of);
        for (LatencyUnit& lu : latency) lu.out_ms = now_ms();
    }
    if (!pipe.latency_log.empty()) {
        std::string js = "{\"units\": [";
        for (size_t i = 0; i < latency.size(); ++i) {
            const LatencyUnit& u = latency[i];
            js += std::string(i ? ", " : "") + "{\"type\": \"" + (u.intra ? "I" : "P") + "\", \"first_picture\": " + std::to_string(u.first_picture) +
                  ", \"pictures\": " + std::to_string(u.pictures) + ", \"qp\": " + std::to_string(u.qp) + ", \"bytes\": " + std::to_string(u.bytes) +
                  ", \"read_ms\": " + jnum(u.read_ms) + ", \"out_ms\": " + jnum(u.out_ms) + "}";
        }
        js += "], \"pictures\": " + std::to_string(frame_num) + ", \"bytes\": " + std::to_string(stream_bytes) + "}\n";
        FILE* lf = fopen(pipe.latency_log.c_str(), "wb");
        if (!lf || fwrite(js.data(), 1, js.size(), lf) != js.size()) die("cannot write " + pipe.latency_log);
        fclose(lf);
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    fprintf(g_msg, "encoded %d pictures (%dx%d) -> %zu bytes, %.4f bpp, %.1f pictures/s (file I/O included)\n", frame_num, g.W, g.H,
            stream_bytes, 8.0 * stream_bytes / (static_cast<double>(frame_num) * g.H * g.W), frame_num / secs);
    if (!input_error.empty()) die(input_error);
    return 0;
}

// The coded stream of decode -i, read front to back through dcvc_stream_next_unit: a regular file, stdin ("-")
// or a FIFO alike. One buffer, grown to the largest need and reused, holds the units of one codec call - one unit, or the I
// units --batch groups - plus the one unit of lookahead the grouping peeks at; every read asks for exactly what next_unit
// says is missing, so nothing behind a unit's end is read before the unit has been decoded.
struct UnitStream {
    int fd = -1;
    std::vector<uint8_t> buf;
    size_t pos = 0, end = 0;       // the read position, and the bytes in the buffer
    bool eof = false;
    void open(const std::string& p)
    {
        fd = is_dash(p) ? 0 : ::open(p.c_str(), O_RDONLY);
        if (fd < 0) die("cannot open " + p);
    }
    // the unit at the read position, whole in memory, without consuming it; false at the clean end of the stream. Truncated
    // and malformed input throw dcvc::stream::StreamError, as the whole-buffer reader does.
    bool peek(dcvc_stream_unit& u)
    {
        for (;;) {
            if (dcvc::stream::next_unit(buf.data() + pos, end - pos, eof, u) > 0) return true;
            if (u.need == 0) return false;
            if (buf.size() < pos + u.need) buf.resize(pos + u.need);
            const ssize_t k = read_upto(fd, buf.data() + end, pos + u.need - end);
            if (k < 0) die(std::string("cannot read the stream: ") + strerror(errno));
            end += static_cast<size_t>(k);
            if (end - pos < u.need) eof = true;
        }
    }
    // what lies in front of the read position has been decoded
    void drop()
    {
        if (pos == 0) return;
        std::memmove(buf.data(), buf.data() + pos, end - pos);
        end -= pos;
        pos = 0;
    }
    void close()
    {
        if (fd > 0) ::close(fd);
        fd = -1;
    }
};

// ------------------------------------------------------------------------------------ decode
int decode(const Args& a)
{
    const int batch = batch_arg(a);
    const SizeArg out_size = size_arg(a, "out-size");
    // MS-SSIM's size floor holds at the size that is measured
    if (out_size.on && a.num("calc-ssim", 0) != 0 && (out_size.H < 176 || out_size.W < 176)) {
        die("--calc-ssim needs both picture sides >= 176 (the chroma planes must be at least 88 x 88 for MS-SSIM), --out-size is " +
            std::to_string(out_size.W) + "x" + std::to_string(out_size.H));
    }
    const PipeArgs pipe = pipe_args(a, false);
    vbv_args(a, batch, false);
    denoise_args(a, false);
    const InterpArgs interp = interp_args(a, false);
    if (interp.on && a.has("verify-hash")) die("--verify-hash checks the decoded pictures against the encoder's manifest: not with --interpolate");
    const GrainArgs grain = grain_args(a, false);
    // the file against what the flags say of the run, before a model is loaded; a Y4M --ref's header is checked against it below
    if (grain.on && !(a.has("ref") && pipe.in_is_y4m(a.str("ref")))) {
        const SrcType t = src_type(a.str("src-type", "yuv420"));
        grain_check_run(grain, src_type_name(t), bit_depth_arg(a, t));
    }
    deinterlace_args(a, false);
    ivtc_args(a, false);
    crop_args(a, false);
    const PadArgs pad = pad_args(a);
    // the log against what the flags say of the run, before a model is loaded; a Y4M --ref's header is checked against it below
    if (pad.on && !(a.has("ref") && pipe.in_is_y4m(a.str("ref")))) {
        const SrcType t = src_type(a.str("src-type", "yuv420"));
        pad_check_run(pad, src_type_name(t), bit_depth_arg(a, t));
    }
    if (a.has("o") && is_dash(a.str("o"))) g_msg = stderr;      // stdout carries the pictures
    // -o *.y4m (or --out-format y4m): what the flags alone decide is refused before a model is loaded
    const bool rec_y4m = a.has("o") && pipe.out_is_y4m(a.str("o"));
    int fps_num = 25, fps_den = 1;
    const bool has_fps = fps_arg(a, fps_num, fps_den);
    if (has_fps && !rec_y4m) die("--fps is the rate in the header of -o *.y4m");
    const ColourArgs colour = colour_args(a);
    HashRun hash;
    hash.parse(a, false);
    const int wire = wire_arg(a, false);
    rgb16_arg(a, false);
    if (rec_y4m) {
        const std::string t = a.str("src-type");
        if (t == "nv12" || t == "p010") die("-o " + a.str("o") + ": Y4M has no tag for interleaved chroma (--src-type " + t + "); write a raw file");
        if (is_rgb_name(t)) die("-o " + a.str("o") + ": a Y4M file holds YUV pictures, not --src-type " + t);
    }
    Codecs c = make_codecs(a.str("intra"), a.str("inter"));
    UnitStream rd;
    rd.open(a.str("i"));
    SrcType type = src_type(a.str("src-type", "yuv420"));
    int depth = bit_depth_arg(a, type);
    const bool has_rec = a.has("o"), has_ref = a.has("ref");
    const bool png = is_png(type);
    // raw or Y4M files (the YUV types, rgb24), or directories of PNG pictures. --ref *.y4m: its header supplies the source
    // type and the bit depth when the flags do not, and must agree with them when they do
    PictureFile ref_file;
    if (has_ref && !png) {
        ref_file.open(a.str("ref"), pipe.in_format);
        if (ref_file.y4m) {
            const Y4mSource y = y4m_source(ref_file, a, false);
            type = y.type; depth = y.depth;
            if (!has_fps) { fps_num = ref_file.info.fps_num; fps_den = ref_file.info.fps_den; }
        }
    }
    const bool rgb = is_rgb(type);
    const int pix_fmt = pix_fmt_of(type);
    if (out_size.on && pix_fmt >= 0) {
        die(std::string("--out-size is for --src-type yuv420: ") + src_type_name(type) + " sources are not resampled yet");
    }
    if (grain.on) grain_check_run(grain, src_type_name(type), depth);
    if (pad.on) pad_check_run(pad, wire >= 0 ? wire_name(wire) : src_type_name(type), depth);
    hash.begin(wire >= 0 ? wire_name(wire) : src_type_name(type), depth);
    FILE* rec = !has_rec || png ? nullptr : is_dash(a.str("o")) ? stdout : fopen(a.str("o").c_str(), "wb");
    if (has_rec && !png && !rec) die("cannot write " + a.str("o"));
    // -o on a pipe ("-", a FIFO): every picture is flushed as it is written; a reader that has gone ends the run with status 1
    const bool rec_piped = rec != nullptr && !fd_is_regular(fileno(rec));
    auto rec_put = [&](const void* p, size_t n) {
        if (fwrite(p, 1, n, rec) == n) return;
        if (errno == EPIPE) output_closed(a.str("o"));
        die("short write");
    };
    auto rec_flush = [&]() {
        if (!rec_piped || fflush(rec) == 0) return;
        if (errno == EPIPE) output_closed(a.str("o"));
        die("short write");
    };
    // -o *.y4m: the header once the first picture's size is known, then a FRAME line in front of every picture
    bool rec_header_done = false;
    auto rec_frame = [&](const Geometry& og) {
        if (!rec_y4m) return;
        if (!rec_header_done) {
            dcvc_y4m_info hi{};
            // --interpolate N: N times the pictures in the same time
            const long long rate = static_cast<long long>(fps_num) * (interp.on ? interp.n : 1);
            if (rate > 2147483647LL) die("--interpolate: the rate of -o *.y4m, " + std::to_string(fps_num) + " times " + std::to_string(interp.n) + ", does not fit its header");
            hi.width = og.W; hi.height = og.H; hi.fps_num = static_cast<int>(rate); hi.fps_den = fps_den;
            hi.pix_fmt = og.pix() ? og.pix_fmt : DCVC_PIX_YUV420P;
            hi.bit_depth = og.bit_depth;
            char line[256];
            const int n = dcvc_y4m_write_header(line, sizeof(line), &hi);
            abi_ok(n, "y4m header");
            rec_put(line, static_cast<size_t>(n));
            rec_header_done = true;
        }
        rec_put("FRAME\n", 6);
    };
    PngDir ref_pngs, rec_pngs;
    if (png && has_ref) ref_pngs = png_dir(a.str("ref"));
    if (png && has_rec) {
        std::error_code fe;
        std::filesystem::create_directories(a.str("o"), fe);
        if (!std::filesystem::is_directory(a.str("o"), fe)) die("cannot create the directory " + a.str("o"));
        rec_pngs.dir = a.str("o");      // the writer's names: im00001.png, ... (video_writer.py:9-30)
    }
    const bool calc_ssim = a.num("calc-ssim", 0) != 0, verbose_json = a.num("verbose-json", 0) != 0;
    if (calc_ssim && !has_ref) die("--calc-ssim needs --ref (the source pictures)");
    const int limit = a.num("n", 1 << 30);
    dcvc::stream::SpsTable sps;
    Geometry g;
    DeviceBuffers b;
    // a wire format: --ref's pictures are unpacked into b.yuv8, where the carrier type's upload lands, and the carrier picture in
    // b.out8 is packed into what -o writes and the hashes cover
    WireStage ws;
    bool have_buffers = false;
    std::vector<uint8_t> src;
    // --out-size: the output pictures' geometry and their buffers, beside the coded size's (which follow the stream)
    Geometry go;
    ScaledOut so;
    if (out_size.on) go = geometry(out_size.H, out_size.W, false, depth);
    // --film-grain / --grain-strength: the grained copy of every output picture, which -o and the hashes see
    GrainSynth gr;
    // --uncrop / --pad: the last stage, shown = pad(grain(resample(picture))): the bars carry no grain
    PadStage pd;
    // --interpolate: in front of both, on the picture the metrics see; its pictures pass through grain, pad, the hashes and -o as
    // a decoded picture does, in output order
    Interpolator ip;
    // cur: the decoded picture at its output size gq; h_w: the pinned buffer -o's pictures of this path leave from
    auto interpolate_to = [&](const Geometry& gq, const uint8_t* cur, uint8_t* h_w) {
        if (ip.begin(cur, b.st)) {
            for (int k = 1; k < interp.n; ++k) {
                const uint8_t* shown = ip.between(cur, k, b.st);
                if (grain.on) shown = gr.run(gq, shown, b.st);
                if (pad.on) shown = pd.run(gq, shown, b.st);
                const Geometry& gw = pad.on ? pd.g : gq;
                if (hash.on()) hash.picture(shown, gw, b.st);
                if (has_rec) {
                    hip_ok(hipMemcpyAsync(h_w, shown, gw.frame_bytes(), hipMemcpyDeviceToHost, b.st), "D2H");
                    hip_ok(hipStreamSynchronize(b.st), "sync");
                    rec_frame(gw);
                    rec_put(h_w, gw.frame_bytes());
                    rec_flush();
                }
            }
        }
        ip.keep(cur, b.st);
    };
    // log (src/utils/common.py:46-116)
    std::vector<int> types;
    std::vector<double> bits, psnr, psnr_y, psnr_u, psnr_v, ssim, ssim_y, ssim_u, ssim_v;
    size_t pending_sps_bits = 0;
    int decoded = 0;
    const auto t0 = std::chrono::steady_clock::now();
    bool source_ended = false;
    if (c.ht && c.frames_per_p > 1 && !a.has("n") && !has_ref) {
        fprintf(stderr, "dcvc: warning: %d-picture chunks and neither -n nor --ref: a short last chunk is written with its "
                        "padding pictures (the container does not carry the picture count)\n", c.frames_per_p);
    }
    while (decoded < limit && !source_ended) {
        rd.drop();                         // the units of the previous codec call leave the buffer
        dcvc_stream_unit u;
        if (!rd.peek(u)) break;
        const size_t payload_at = rd.pos + u.payload_offset;
        rd.pos += u.unit_bytes;
        const int nal = u.nal_type, sid = u.sps_id;
        if (nal == dcvc::stream::kSps) {
            sps.add(sid, u.height, u.width);
            pending_sps_bits += 8 * u.unit_bytes;
            continue;
        }
        const dcvc::stream::SpsTable::Sps* s = sps.find(sid);
        if (!s) die("picture refers to an unknown parameter set");
        if (!have_buffers || s->height != g.H || s->width != g.W) {
            // the size comes straight from the (untrusted) stream: refuse what no model of this family codes
            // instead of attempting a multi-terabyte allocation
            if (s->height < 2 || s->width < 2 || s->height > kMaxPictureSide || s->width > kMaxPictureSide) {
                die("unsupported picture size in the stream: " + std::to_string(s->width) + "x" + std::to_string(s->height));
            }
            // MS-SSIM needs both sides of every plane >= 88 (metrics.py asserts): refused before anything is decoded
            if (calc_ssim && rgb && (s->height < 88 || s->width < 88)) {
                die("--calc-ssim needs both picture sides >= 88 (MS-SSIM of the R, G and B planes), the stream holds " +
                    std::to_string(s->width) + "x" + std::to_string(s->height));
            }
            if (calc_ssim && pix_fmt >= 0) {
                const Geometry t = geometry(s->height, s->width, false, depth, pix_fmt);
                if (t.H < 88 || t.W < 88 || t.Hc() < 88 || t.Wc() < 88) {
                    die("--calc-ssim needs the sides of every plane >= 88 (MS-SSIM of the Y, Cb and Cr planes), the stream holds " +
                        std::to_string(s->width) + "x" + std::to_string(s->height) + " with " + std::to_string(t.Wc()) + "x" +
                        std::to_string(t.Hc()) + " chroma planes");
                }
            }
            if (ref_file.y4m && (ref_file.info.width != (out_size.on ? out_size.W : s->width) ||
                                 ref_file.info.height != (out_size.on ? out_size.H : s->height))) {
                die(ref_file.path + " holds " + std::to_string(ref_file.info.width) + "x" + std::to_string(ref_file.info.height) +
                    " pictures, the output is " + std::to_string(out_size.on ? out_size.W : s->width) + "x" +
                    std::to_string(out_size.on ? out_size.H : s->height));
            }
            if (calc_ssim && !rgb && pix_fmt < 0 && !out_size.on && (s->height < 176 || s->width < 176)) {
                die("--calc-ssim needs both picture sides >= 176 (the chroma planes must be at least 88 x 88 for MS-SSIM), the "
                    "stream holds " + std::to_string(s->width) + "x" + std::to_string(s->height));
            }
            if (out_size.on) check_ratio("--out-size", s->width, s->height, go.W, go.H);
            if (grain.from_file && !out_size.on && (grain.file.width != s->width || grain.file.height != s->height)) {
                die("--film-grain: the file describes " + std::to_string(grain.file.width) + "x" + std::to_string(grain.file.height) +
                    " pictures, the stream holds " + std::to_string(s->width) + "x" + std::to_string(s->height));
            }
            if (pad.on) {
                // the picture arriving at the stage must be the window; -o and the hashes hold the source's size
                pd.create(pad, out_size.on ? go : geometry(s->height, s->width, rgb, depth, pix_fmt, wire));
                hash.size(pd.g.W, pd.g.H);
            } else {
                hash.size(out_size.on ? go.W : s->width, out_size.on ? go.H : s->height);
            }
            if (have_buffers && ip.active) ip.flush(b.st);
            if (have_buffers) free_buffers(b);     // a stream may switch parameter sets: do not leak the old set
            g = geometry(s->height, s->width, rgb, depth, pix_fmt, wire);
            if (rgb) colour.apply(g);
            b = make_buffers(g, std::max(c.frames_per_p, batch), calc_ssim);
            ws.create(g);
            if (out_size.on) so.create(g, go, has_ref, calc_ssim);
            if (grain.on) gr.create(out_size.on ? go : g, grain);
            if (interp.on) ip.create(interp, out_size.on ? go : g, pipe.in_format);
            src.resize(g.frame_bytes());
            have_buffers = true;
        }
        const int qp = u.qp, ec = u.ec_part;
        const bool reset = u.reset != 0;
        const size_t n = u.payload_bytes;
        const bool intra = nal == dcvc::stream::kIntra;
        int frames = 1;
        // bits of each picture's unit (an 8-picture chunk: all on its first picture); a new parameter set counts with the next unit
        std::vector<double> unit_bits{8.0 * u.unit_bytes + pending_sps_bits};
        pending_sps_bits = 0;
        if (intra && batch > 1) {
            // --batch: this and up to batch - 1 following I units of the same size and qp in one call (a parameter set, a P unit,
            // another size or qp ends the group). The buffer may move while it takes the next unit in: offsets until the call.
            std::vector<size_t> at{payload_at};
            std::vector<size_t> sizes{n};
            std::vector<int> ecs{ec};
            while (static_cast<int>(at.size()) < batch && decoded + static_cast<int>(at.size()) < limit) {
                dcvc_stream_unit u2;
                try {
                    if (!rd.peek(u2)) break;
                } catch (const std::exception&) {
                    break;              // a malformed unit: the single path below reports it
                }
                if (u2.nal_type != dcvc::stream::kIntra) break;
                const dcvc::stream::SpsTable::Sps* s2 = sps.find(u2.sps_id);
                if (s2 == nullptr || s2->height != g.H || s2->width != g.W) break;
                if (u2.qp != qp) break;
                at.push_back(rd.pos + u2.payload_offset); sizes.push_back(u2.payload_bytes); ecs.push_back(u2.ec_part);
                rd.pos += u2.unit_bytes;
                unit_bits.push_back(8.0 * u2.unit_bytes);
            }
            std::vector<const uint8_t*> pls;
            for (size_t off : at) pls.push_back(rd.buf.data() + off);
            frames = static_cast<int>(pls.size());
            abi_ok(dcvc_dmci_decompress_batch(c.intra, frames, pls.data(), sizes.data(), ecs.data(), qp, g.H, g.W, b.x_hat, b.st),
                   "intra decompress");
            for (int j = 0; j < frames; ++j) {
                const char* xh = static_cast<const char*>(b.x_hat) + static_cast<size_t>(j) * g.Hp * g.Wp * 3 * 2;
                if (c.ld) abi_ok(dcvc_dmcld_add_ref_feature_from_frame(c.ld, xh, g.Hp, g.Wp, 0, b.st), "add_ref");
                if (c.ht) abi_ok(dcvc_dmcht_add_ref_feature_from_frame(c.ht, xh, g.Hp, g.Wp, 0, b.st), "add_ref");
            }
        } else if (intra) {
            abi_ok(dcvc_dmci_decompress(c.intra, rd.buf.data() + payload_at, n, qp, g.H, g.W, ec, b.x_hat, b.st), "intra decompress");
            if (c.ld) abi_ok(dcvc_dmcld_add_ref_feature_from_frame(c.ld, b.x_hat, g.Hp, g.Wp, 0, b.st), "add_ref");
            if (c.ht) abi_ok(dcvc_dmcht_add_ref_feature_from_frame(c.ht, b.x_hat, g.Hp, g.Wp, 0, b.st), "add_ref");
        } else if (c.ld) {
            abi_ok(dcvc_dmcld_decompress(c.ld, rd.buf.data() + payload_at, n, qp, g.H, g.W, ec, reset ? 1 : 0, b.x_hat, b.st), "inter decompress");
        } else if (c.ht) {
            abi_ok(dcvc_dmcht_decompress(c.ht, rd.buf.data() + payload_at, n, qp, g.H, g.W, ec, reset ? 1 : 0, b.x_hat, b.st), "inter decompress");
            frames = c.frames_per_p;
        } else {
            die("the stream holds P pictures but no inter model was given");
        }
        for (int j = 0; j < frames && decoded < limit; ++j) {
            const char* xh = static_cast<const char*>(b.x_hat) + static_cast<size_t>(j) * g.Hp * g.Wp * 3 * 2;
            char* y16 = static_cast<char*>(b.y16);
            // --hash-log / --verify-hash without -o: the samples are wanted on the device although nothing is written
            x_hat_to_picture(g, b, xh, g.hbd() && !g.pix() ? has_rec || out_size.on || hash.on() || interp.on : has_rec || hash.on() || interp.on);
            if (out_size.on) {
                // b.out8 holds the integer samples -o would write at the coded size: resample them, then the output picture is
                // written and measured at its own size, sample against sample (the source first, as below)
                const size_t ny = go.y_bytes(), nc = ny / 4, es = go.hbd() ? 2 : 1;
                if (has_ref && !ref_file.read(so.h_ref, go.frame_bytes())) {
                    if (j > 0 && !intra) { source_ended = true; break; }
                    die("reference file is shorter than the stream");
                }
                so.rs.run(b.out8, so.out, b.st);
                if (interp.on) interpolate_to(go, so.out, pad.on ? pd.h_out : so.h_out);
                // the metrics below read so.out, the ungrained picture
                const uint8_t* shown = grain.on ? gr.run(go, so.out, b.st) : so.out;
                if (pad.on) shown = pd.run(go, shown, b.st);
                const Geometry& gw = pad.on ? pd.g : go;      // what -o writes and the hashes cover
                uint8_t* const h_w = pad.on ? pd.h_out : so.h_out;
                if (hash.on()) hash.picture(shown, gw, b.st);
                if (has_rec) hip_ok(hipMemcpyAsync(h_w, shown, gw.frame_bytes(), hipMemcpyDeviceToHost, b.st), "D2H");
                if (has_ref) {
                    const int dt = go.hbd() ? DCVC_SAMPLE_U16 : DCVC_SAMPLE_U8;
                    const double peak = static_cast<double>((1 << go.bit_depth) - 1);
                    hip_ok(hipMemcpyAsync(so.ref, so.h_ref, go.frame_bytes(), hipMemcpyHostToDevice, b.st), "H2D");
                    abi_ok(dcvc_sse_ws(so.ref, dt, so.out, dt, 1, go.H, go.W, go.W, static_cast<long long>(ny), so.sse, so.sse_ws,
                                       so.sse_ws_bytes, b.st), "sse (Y)");
                    abi_ok(dcvc_sse_ws(so.ref + ny * es, dt, so.out + ny * es, dt, 2, go.H / 2, go.W / 2, go.W / 2, static_cast<long long>(nc),
                                       so.sse + 1, so.sse_ws, so.sse_ws_bytes, b.st), "sse (U, V)");
                    hip_ok(hipMemcpyAsync(so.h_sse, so.sse, 3 * sizeof(double), hipMemcpyDeviceToHost, b.st), "D2H");
                    if (calc_ssim) {
                        // data_range 255 gives dcvc_msssim's bits; the workspace is the tool's own, as for the sums
                        abi_ok(dcvc_msssim_range_ws(so.ref, dt, so.out, dt, 1, go.H, go.W, go.W, static_cast<long long>(ny), peak, so.ssim,
                                                    so.ssim_ws, so.ssim_ws_bytes, b.st), "msssim (Y)");
                        abi_ok(dcvc_msssim_range_ws(so.ref + ny * es, dt, so.out + ny * es, dt, 2, go.H / 2, go.W / 2, go.W / 2,
                                                    static_cast<long long>(nc), peak, so.ssim + 1, so.ssim_ws, so.ssim_ws_bytes, b.st),
                               "msssim (U, V)");
                    }
                    if (calc_ssim) hip_ok(hipMemcpyAsync(so.h_ssim, so.ssim, 3 * sizeof(double), hipMemcpyDeviceToHost, b.st), "D2H");
                    hip_ok(hipStreamSynchronize(b.st), "sync");
                    const double py = psnr_of_sse(so.h_sse[0], static_cast<double>(ny), peak);
                    const double pu = psnr_of_sse(so.h_sse[1], static_cast<double>(nc), peak);
                    const double pv = psnr_of_sse(so.h_sse[2], static_cast<double>(nc), peak);
                    psnr.push_back((6 * py + pu + pv) / 8); psnr_y.push_back(py); psnr_u.push_back(pu); psnr_v.push_back(pv);
                    if (calc_ssim) {
                        const double sy = so.h_ssim[0], su = so.h_ssim[1], sv = so.h_ssim[2];
                        ssim.push_back((6 * sy + su + sv) / 8); ssim_y.push_back(sy); ssim_u.push_back(su); ssim_v.push_back(sv);
                    }
                }
                if (has_rec) {
                    hip_ok(hipStreamSynchronize(b.st), "sync");
                    rec_frame(gw);
                    rec_put(h_w, gw.frame_bytes());
                    rec_flush();
                }
                types.push_back(intra ? 0 : 1);
                bits.push_back(j < static_cast<int>(unit_bits.size()) ? unit_bits[static_cast<size_t>(j)] : 0.0);
                ++decoded;
                continue;
            }
            // the source first: when it ends inside a chunk, the remaining pictures of the chunk are the encoder's
            // padding (repeats of the final picture) and must reach neither the log nor rec.yuv
            if (has_ref) {
                uint8_t* sp = wire >= 0 ? ws.h_in : rgb || g.hbd() || g.pix() ? b.h_src : src.data();      // RGB, high bit depth: straight into pinned memory
                const bool got = png ? ref_pngs.read(sp, g) : ref_file.read(sp, g.file_bytes());
                if (!got) {
                    if (j > 0 && !intra) { source_ended = true; break; }      // (an I batch: as its pictures one by one)
                    die("reference file is shorter than the stream");
                }
            }
            if (wire >= 0 && (has_rec || hash.on())) ws.pack(g, b.out8, b.st);
            // grain behind the source check above: a padding picture of a ragged chunk takes no picture index
            if (interp.on) interpolate_to(g, b.out8, pad.on ? pd.h_out : b.h_yuv);
            const uint8_t* shown = grain.on ? gr.run(g, b.out8, b.st) : b.out8;
            if (pad.on) shown = pd.run(g, shown, b.st);        // (no wire format, no RGB: refused above)
            const Geometry& gw = pad.on ? pd.g : g;            // what -o writes and the hashes cover
            uint8_t* const h_w = pad.on ? pd.h_out : b.h_yuv;
            if (hash.on()) hash.picture(wire >= 0 ? ws.out : shown, gw, b.st);
            if (has_rec && wire >= 0) {
                hip_ok(hipMemcpyAsync(ws.h_out, ws.out, g.file_bytes(), hipMemcpyDeviceToHost, b.st), "D2H");
                hip_ok(hipStreamSynchronize(b.st), "sync");
                rec_put(ws.h_out, g.file_bytes());
                rec_flush();
            } else if (has_rec) {
                hip_ok(hipMemcpyAsync(h_w, shown, gw.frame_bytes(), hipMemcpyDeviceToHost, b.st), "D2H");
                hip_ok(hipStreamSynchronize(b.st), "sync");
                if (png && g.rgb16()) {
                    abi_ok(dcvc_png_write_rgb16(rec_pngs.path(rec_pngs.next++).c_str(), b.h_yuv, g.W, g.H), "png write");
                } else if (png) {
                    abi_ok(dcvc_png_write_rgb(rec_pngs.path(rec_pngs.next++).c_str(), b.h_yuv, g.W, g.H), "png write");
                } else {
                    rec_frame(gw);
                    rec_put(h_w, gw.frame_bytes());
                    rec_flush();
                }
            }
            if (has_ref && g.rgb16()) {
                // the RGB branch below at 9..16 bits: the source's planar u16 copy against the fp32 planes, data range max_val;
                // MS-SSIM plane by plane on the tool's own workspace
                const size_t plane = g.y_bytes();
                const double peak = static_cast<double>((1 << g.bit_depth) - 1);
                hip_ok(hipMemcpyAsync(b.yuv8, b.h_src, g.frame_bytes(), hipMemcpyHostToDevice, b.st), "H2D");
                abi_ok(dcvc_rgb16_to_x_cs(b.yuv8, 3LL * g.W, 3, 1, g.bit_depth, g.H, g.W, nullptr, 3, b.src8, g.matrix, g.range, g.yuv_depth,
                                          b.st), "rgb16_to_x_cs (planar source)");
                abi_ok(dcvc_sse_ws(b.src8, DCVC_SAMPLE_U16, y16, DCVC_SAMPLE_F32, 3, g.H, g.W, g.W, static_cast<long long>(plane), b.sse,
                                   b.sse_ws, b.sse_ws_bytes, b.st), "sse");
                hip_ok(hipMemcpyAsync(b.h_sse, b.sse, 3 * sizeof(double), hipMemcpyDeviceToHost, b.st), "D2H");
                if (calc_ssim) {
                    for (size_t q = 0; q < 3; ++q) {
                        abi_ok(dcvc_msssim_range_ws(b.src8 + q * plane * 2, DCVC_SAMPLE_U16, y16 + q * plane * 4, DCVC_SAMPLE_F32, 1, g.H, g.W,
                                                    g.W, static_cast<long long>(plane), peak, b.ssim + q, b.ssim_ws, b.ssim_ws_bytes, b.st),
                               "msssim (R, G, B)");
                    }
                    hip_ok(hipMemcpyAsync(b.h_ssim, b.ssim, 3 * sizeof(double), hipMemcpyDeviceToHost, b.st), "D2H");
                }
                hip_ok(hipStreamSynchronize(b.st), "sync");
                psnr.push_back(psnr_of_sse((b.h_sse[0] + b.h_sse[1]) + b.h_sse[2], 3.0 * static_cast<double>(plane), peak));
                if (calc_ssim) ssim.push_back(((0.0 + b.h_ssim[0]) + b.h_ssim[1] + b.h_ssim[2]) / 3);
            } else if (has_ref && rgb) {
                // get_distortion (png branch): calc_psnr over the 3 H W samples from the device's sums of squares; the
                // source's planar copy next to the fp16 planes for dcvc_sse and dcvc_msssim
                // (the copy leaves from pinned memory, and the workspace is the tool's own: nothing in this loop depends on
                // how the runtime stages a pageable copy or recycles a stream-ordered allocation)
                const size_t plane = g.y_bytes();
                hip_ok(hipMemcpyAsync(b.yuv8, b.h_src, g.frame_bytes(), hipMemcpyHostToDevice, b.st), "H2D");
                abi_ok(dcvc_rgb_to_x_cs(b.yuv8, 3LL * g.W, 3, 1, g.H, g.W, nullptr, 3, b.src8, g.matrix, g.range, g.yuv_depth, b.st),
                       "rgb_to_x_cs (planar source)");
                abi_ok(dcvc_sse_ws(b.src8, DCVC_SAMPLE_U8, y16, DCVC_SAMPLE_F16, 3, g.H, g.W, g.W, static_cast<long long>(plane), b.sse,
                                   b.sse_ws, b.sse_ws_bytes, b.st), "sse");
                hip_ok(hipMemcpyAsync(b.h_sse, b.sse, 3 * sizeof(double), hipMemcpyDeviceToHost, b.st), "D2H");
                if (calc_ssim) {
                    abi_ok(dcvc_msssim(b.src8, DCVC_SAMPLE_U8, y16, DCVC_SAMPLE_F16, 3, g.H, g.W, g.W, static_cast<long long>(plane),
                                       b.ssim, b.st), "msssim (R, G, B)");
                    hip_ok(hipMemcpyAsync(b.h_ssim, b.ssim, 3 * sizeof(double), hipMemcpyDeviceToHost, b.st), "D2H");
                }
                hip_ok(hipStreamSynchronize(b.st), "sync");
                psnr.push_back(psnr_of_sse((b.h_sse[0] + b.h_sse[1]) + b.h_sse[2], 3.0 * static_cast<double>(plane)));
                if (calc_ssim) ssim.push_back(((0.0 + b.h_ssim[0]) + b.h_ssim[1] + b.h_ssim[2]) / 3);    // calc_msssim_rgb
            } else if (has_ref && g.pix()) {
                // the other chroma formats, at every depth: the source as LSB-aligned planar samples (dcvc_pix_to_x's planar
                // output, from the pinned picture) against dcvc_x_to_pix's fp32 planes, summed and measured on the device
                const size_t ny = g.y_bytes(), nc = static_cast<size_t>(g.Hc()) * g.Wc(), es = g.hbd() ? 2 : 1;
                const int dt = g.hbd() ? DCVC_SAMPLE_U16 : DCVC_SAMPLE_U8;
                const double peak = static_cast<double>((1 << g.bit_depth) - 1);
                const uint8_t* src_uv = b.src8 + ny * es;
                const char* dist_uv = y16 + ny * 4;
                if (wire >= 0) ws.upload(g, b.yuv8, b.st);
                else hip_ok(hipMemcpyAsync(b.yuv8, b.h_src, g.frame_bytes(), hipMemcpyHostToDevice, b.st), "H2D");
                abi_ok(dcvc_pix_to_x(b.yuv8, g.pix_fmt, g.bit_depth, g.H, g.W, nullptr, 3, b.src8, b.st), "pix_to_x (planar source)");
                abi_ok(dcvc_sse_ws(b.src8, dt, y16, DCVC_SAMPLE_F32, 1, g.H, g.W, g.W, static_cast<long long>(ny), b.sse, b.sse_ws,
                                   b.sse_ws_bytes, b.st), "sse (Y)");
                abi_ok(dcvc_sse_ws(src_uv, dt, dist_uv, DCVC_SAMPLE_F32, 2, g.Hc(), g.Wc(), g.Wc(), static_cast<long long>(nc), b.sse + 1,
                                   b.sse_ws, b.sse_ws_bytes, b.st), "sse (U, V)");
                hip_ok(hipMemcpyAsync(b.h_sse, b.sse, 3 * sizeof(double), hipMemcpyDeviceToHost, b.st), "D2H");
                if (calc_ssim) {
                    abi_ok(dcvc_msssim_range_ws(b.src8, dt, y16, DCVC_SAMPLE_F32, 1, g.H, g.W, g.W, static_cast<long long>(ny), peak, b.ssim,
                                                b.ssim_ws, b.ssim_ws_bytes, b.st), "msssim (Y)");
                    abi_ok(dcvc_msssim_range_ws(src_uv, dt, dist_uv, DCVC_SAMPLE_F32, 2, g.Hc(), g.Wc(), g.Wc(), static_cast<long long>(nc), peak,
                                                b.ssim + 1, b.ssim_ws, b.ssim_ws_bytes, b.st), "msssim (U, V)");
                    hip_ok(hipMemcpyAsync(b.h_ssim, b.ssim, 3 * sizeof(double), hipMemcpyDeviceToHost, b.st), "D2H");
                }
                hip_ok(hipStreamSynchronize(b.st), "sync");
                const double py = psnr_of_sse(b.h_sse[0], static_cast<double>(ny), peak);
                const double pu = psnr_of_sse(b.h_sse[1], static_cast<double>(nc), peak);
                const double pv = psnr_of_sse(b.h_sse[2], static_cast<double>(nc), peak);
                // (6 Y + U + V) / 8 for every format: this tool's convention beyond 4:2:0, where the reference defines it
                psnr.push_back((6 * py + pu + pv) / 8); psnr_y.push_back(py); psnr_u.push_back(pu); psnr_v.push_back(pv);
                if (calc_ssim) {
                    const double sy = b.h_ssim[0], su = b.h_ssim[1], sv = b.h_ssim[2];
                    ssim.push_back((6 * sy + su + sv) / 8); ssim_y.push_back(sy); ssim_u.push_back(su); ssim_v.push_back(sv);
                }
            } else if (has_ref && g.hbd()) {
                // as the RGB branch: sums of squares and MS-SSIM on the device from the pinned source, data range max_val
                const size_t ny = g.y_bytes(), nc = ny / 4;
                const double peak = static_cast<double>((1 << g.bit_depth) - 1);
                const uint8_t* src_uv = b.src8 + ny * 2;
                const char* dist_uv = y16 + ny * 4;
                hip_ok(hipMemcpyAsync(b.src8, b.h_src, g.frame_bytes(), hipMemcpyHostToDevice, b.st), "H2D");
                abi_ok(dcvc_sse_ws(b.src8, DCVC_SAMPLE_U16, y16, DCVC_SAMPLE_F32, 1, g.H, g.W, g.W, static_cast<long long>(ny), b.sse,
                                   b.sse_ws, b.sse_ws_bytes, b.st), "sse (Y)");
                abi_ok(dcvc_sse_ws(src_uv, DCVC_SAMPLE_U16, dist_uv, DCVC_SAMPLE_F32, 2, g.H / 2, g.W / 2, g.W / 2, static_cast<long long>(nc),
                                   b.sse + 1, b.sse_ws, b.sse_ws_bytes, b.st), "sse (U, V)");
                hip_ok(hipMemcpyAsync(b.h_sse, b.sse, 3 * sizeof(double), hipMemcpyDeviceToHost, b.st), "D2H");
                if (calc_ssim) {
                    abi_ok(dcvc_msssim_range(b.src8, DCVC_SAMPLE_U16, y16, DCVC_SAMPLE_F32, 1, g.H, g.W, g.W, static_cast<long long>(ny),
                                             peak, b.ssim, b.st), "msssim (Y)");
                    abi_ok(dcvc_msssim_range(src_uv, DCVC_SAMPLE_U16, dist_uv, DCVC_SAMPLE_F32, 2, g.H / 2, g.W / 2, g.W / 2,
                                             static_cast<long long>(nc), peak, b.ssim + 1, b.st), "msssim (U, V)");
                    hip_ok(hipMemcpyAsync(b.h_ssim, b.ssim, 3 * sizeof(double), hipMemcpyDeviceToHost, b.st), "D2H");
                }
                hip_ok(hipStreamSynchronize(b.st), "sync");
                const double py = psnr_of_sse(b.h_sse[0], static_cast<double>(ny), peak);
                const double pu = psnr_of_sse(b.h_sse[1], static_cast<double>(nc), peak);
                const double pv = psnr_of_sse(b.h_sse[2], static_cast<double>(nc), peak);
                psnr.push_back((6 * py + pu + pv) / 8); psnr_y.push_back(py); psnr_u.push_back(pu); psnr_v.push_back(pv);
                if (calc_ssim) {
                    const double sy = b.h_ssim[0], su = b.h_ssim[1], sv = b.h_ssim[2];
                    ssim.push_back((6 * sy + su + sv) / 8); ssim_y.push_back(sy); ssim_u.push_back(su); ssim_v.push_back(sv);
                }
            } else if (has_ref) {
                const size_t ny = g.y_bytes(), nc = ny / 4;
                if (calc_ssim) {
                    // the source picture next to the decoded fp16 planes; Y as one plane, U + V as two
                    hip_ok(hipMemcpyAsync(b.src8, src.data(), g.frame_bytes(), hipMemcpyHostToDevice, b.st), "H2D");
                    abi_ok(dcvc_msssim(b.src8, DCVC_SAMPLE_U8, y16, DCVC_SAMPLE_F16, 1, g.H, g.W, g.W, static_cast<long long>(ny), b.ssim,
                                       b.st), "msssim (Y)");
                    abi_ok(dcvc_msssim(b.src8 + ny, DCVC_SAMPLE_U8, y16 + ny * 2, DCVC_SAMPLE_F16, 2, g.H / 2, g.W / 2, g.W / 2,
                                       static_cast<long long>(nc), b.ssim + 1, b.st), "msssim (U, V)");
                    hip_ok(hipMemcpyAsync(b.h_ssim, b.ssim, 3 * sizeof(double), hipMemcpyDeviceToHost, b.st), "D2H");
                }
                hip_ok(hipMemcpyAsync(b.h_p16, b.y16, g.frame_bytes() * 2, hipMemcpyDeviceToHost, b.st), "D2H");
                hip_ok(hipStreamSynchronize(b.st), "sync");
                const double py = psnr_plane(src.data(), b.h_p16, ny);
                const double pu = psnr_plane(src.data() + ny, b.h_p16 + ny, nc);
                const double pv = psnr_plane(src.data() + ny + nc, b.h_p16 + ny + nc, nc);
                psnr.push_back((6 * py + pu + pv) / 8); psnr_y.push_back(py); psnr_u.push_back(pu); psnr_v.push_back(pv);
                if (calc_ssim) {
                    const double sy = b.h_ssim[0], su = b.h_ssim[1], sv = b.h_ssim[2];
                    ssim.push_back((6 * sy + su + sv) / 8); ssim_y.push_back(sy); ssim_u.push_back(su); ssim_v.push_back(sv);
                }
            }
            types.push_back(intra ? 0 : 1);
            bits.push_back(j < static_cast<int>(unit_bits.size()) ? unit_bits[static_cast<size_t>(j)] : 0.0);
            ++decoded;
        }
    }
    const std::string interp_tail = ip.finish(b.st);
    if (have_buffers) free_buffers(b);
    ws.destroy();
    so.destroy();
    gr.destroy();
    pd.destroy();
    ip.destroy();
    if (rec && fclose(rec) != 0) {
        if (errno == EPIPE) output_closed(a.str("o"));
        die("short write");
    }
    ref_file.close();
    rd.close();
    hash.finish();
    const int nk = rgb ? 1 : 4;        // the RGB log has no _y / _u / _v keys (common.py:46-116 without include_yuv)
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (out_size.on) {
        fprintf(g_msg, "decoded %d pictures (%dx%d, output at %dx%d), %.1f pictures/s (file I/O included)%s\n", decoded, g.W, g.H, go.W, go.H,
                decoded / secs, interp_tail.c_str());
    } else {
        fprintf(g_msg, "decoded %d pictures (%dx%d), %.1f pictures/s (file I/O included)%s\n", decoded, g.W, g.H, decoded / secs, interp_tail.c_str());
    }
    if (a.has("json")) {
        if (psnr.size() != types.size()) die("--json needs --ref (PSNR per picture)");
        const double px = out_size.on ? static_cast<double>(go.H) * go.W : static_cast<double>(g.H) * g.W;
        double ib = 0, pb = 0, ip[4] = {0, 0, 0, 0}, pp[4] = {0, 0, 0, 0};
        int ni = 0, np = 0;
        for (size_t i = 0; i < types.size(); ++i) {
            double* t = types[i] == 0 ? ip : pp;
            (types[i] == 0 ? ib : pb) += bits[i];
            (types[i] == 0 ? ni : np) += 1;
            t[0] += psnr[i];
            if (!rgb) { t[1] += psnr_y[i]; t[2] += psnr_u[i]; t[3] += psnr_v[i]; }
        }
        FILE* jf = fopen(a.str("json").c_str(), "w");
        if (!jf) die("cannot write " + a.str("json"));
        const char* sfx[4] = {"", "_y", "_u", "_v"};
        fprintf(jf, "{\n  \"arith_policy\": %d,\n  \"frame_pixel_num\": %.0f,\n  \"i_frame_num\": %d,\n  \"p_frame_num\": %d,\n", dcvc_arith_policy_version(), px, ni, np);
        if (out_size.on) fprintf(jf, "  \"coded_width\": %d,\n  \"coded_height\": %d,\n", g.W, g.H);
        if (colour.on) {
            fprintf(jf, "  \"color_matrix\": \"%s\",\n  \"color_range\": \"%s\",\n  \"color_yuv_depth\": %d,\n", colour.matrix_name.c_str(),
                    colour.range_name.c_str(), colour.yuv_depth);
        }
        fprintf(jf, "  \"ave_i_frame_bpp\": %.9g,\n  \"ave_p_frame_bpp\": %.9g,\n", ni ? ib / ni / px : 0.0, np ? pb / np / px : 0.0);
        if (rgb) {
            // 17 digits, as Python's json writes a float (the YUV log keeps its 9)
            fprintf(jf, "  \"ave_i_frame_psnr\": %s,\n  \"ave_p_frame_psnr\": %s,\n  \"ave_all_frame_psnr\": %s,\n",
                    jnum(ni ? ip[0] / ni : 0.0).c_str(), jnum(np ? pp[0] / np : 0.0).c_str(), jnum((ip[0] + pp[0]) / std::max(1, ni + np)).c_str());
        } else {
            for (int k = 0; k < 4; ++k) {
                fprintf(jf, "  \"ave_i_frame_psnr%s\": %.9g,\n  \"ave_p_frame_psnr%s\": %.9g,\n  \"ave_all_frame_psnr%s\": %.9g,\n", sfx[k],
                        ni ? ip[k] / ni : 0.0, sfx[k], np ? pp[k] / np : 0.0, sfx[k], (ip[k] + pp[k]) / std::max(1, ni + np));
            }
        }
        if (calc_ssim) {
            // common.py:78-114: the i / p / all averages of (6 y + u + v) / 8 and of each plane (0 for an empty class)
            const std::vector<double>* sv[4] = {&ssim, &ssim_y, &ssim_u, &ssim_v};
            for (int k = 0; k < nk; ++k) {
                double si = 0, sp = 0;
                for (size_t i = 0; i < types.size(); ++i) (types[i] == 0 ? si : sp) += (*sv[k])[i];
                fprintf(jf, "  \"ave_i_frame_msssim%s\": %s,\n  \"ave_p_frame_msssim%s\": %s,\n  \"ave_all_frame_msssim%s\": %s,\n",
                        sfx[k], jnum(ni ? si / ni : 0.0).c_str(), sfx[k], jnum(np ? sp / np : 0.0).c_str(), sfx[k],
                        jnum((si + sp) / std::max(1, ni + np)).c_str());
            }
        }
        if (verbose_json) {
            // common.py:90-98
            std::vector<double> bpp(bits.size());
            for (size_t i = 0; i < bits.size(); ++i) bpp[i] = bits[i] / px;
            std::string ft = "[";
            for (size_t i = 0; i < types.size(); ++i) ft += (i ? ", " : "") + std::to_string(types[i]);
            ft += "]";
            fprintf(jf, "  \"frame_bpp\": %s,\n  \"frame_type\": %s,\n", jlist(bpp).c_str(), ft.c_str());
            const std::vector<double>* pv[4] = {&psnr, &psnr_y, &psnr_u, &psnr_v};
            const std::vector<double>* mv[4] = {&ssim, &ssim_y, &ssim_u, &ssim_v};
            for (int k = 0; k < nk; ++k) {
                fprintf(jf, "  \"frame_psnr%s\": %s,\n", sfx[k], jlist(*pv[k]).c_str());
                if (calc_ssim) fprintf(jf, "  \"frame_msssim%s\": %s,\n", sfx[k], jlist(*mv[k]).c_str());
            }
        }
        fprintf(jf, "  \"ave_all_frame_bpp\": %.9g,\n  \"test_time\": %.3f\n}\n", (ib + pb) / (std::max(1, ni + np) * px), secs);
        fclose(jf);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    // one hardware queue per stream-priority level, before the HIP runtime starts ("Runtime settings":
    // with ROCclr's default of 4 the throughput of several codec objects in one process depends on their creation order);
    // a value in the environment wins
    setenv("GPU_MAX_HW_QUEUES", "1", 0);
    // a pipe whose reader has gone: the write fails with EPIPE and the run ends with status 1 and one line (output_closed)
    signal(SIGPIPE, SIG_IGN);
    if (argc < 2) die("usage: dcvc encode|decode ... (see the head of dcvc_cli.hip)");
    const std::string mode = argv[1];
    try {
        const Args a = parse(argc, argv);
        if (!a.has("intra") || !a.has("i")) die("--intra and -i are required");
        if (mode == "encode") {
            if (!a.has("o")) die("-o is required");
            return encode(a);
        }
        if (mode == "decode") return decode(a);
    } catch (const std::exception& e) {
        die(e.what());
    }
    die("unknown mode " + mode);
}
