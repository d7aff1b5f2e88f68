// TypeScript surface of the Node host (tsc is not part of the build image; this file is the typed contract).
/// <reference types="node" />
export type Direction = 'vertical' | 'horizontal';
export type StitchMode = 'min' | 'max' | 'original';
export type ColorProfile = 'ignore' | 'srgb';
export interface StitchImage {
  width: number;            // naturalWidth  (pages/index/index.js:724-739)
  height: number;           // naturalHeight
  data?: Uint8Array;        // RGBA8, straight alpha, row-major, width*height*4 bytes
  orientation?: 1 | 2 | 3 | 4 | 5 | 6 | 7 | 8;
  fileSize?: number;        // bytes, feeds bigTask (index.js:1211-1212)
  opaque?: boolean;         // hint: all alpha bytes are 255
  bmpWidth?: number; bmpHeight?: number;
}
export interface StitchOptions {
  mode?: StitchMode; gap?: number; filter?: 'bilinear' | 'nearest' | 'area' | 'cubic';      // 'area': box-average minified axes (one reading of imageSmoothingQuality 'high'); 'cubic': Catmull-Rom on axes that do not shrink, the box of 'area' on those that do; default bilinear
  platform?: 'ios' | 'android' | 'devtools' | 'windows' | 'mac' | 'other';
  maxSide?: number; maxPixels?: number; superSample?: number;
  edgeAA?: boolean;                         // anti-alias fractional rectangle edges (ctx.scale(superSample), unrounded cursor); default: true iff `platform` is given
  onProgress?: (percent: number) => void;   // stitchProgress checkpoints (index.js:1193-1611)
  pngLevel?: 0 | 1;                         // PNG export form: 0 stored, 1 compressed on the GPU (process-wide once set)
  colorProfile?: ColorProfile;              // stitchFiles only (decodeBitmaps takes its own): 'srgb' converts files tagged with a matrix/TRC ICC profile (Display P3, Adobe RGB) to sRGB on the GPU behind their decode; default 'ignore'
  pngMatch?: 'run' | 'window';              // PNG matches: 'run' runs inside a 64-byte span (default), 'window' a chunk also copies from its earlier spans, found on the GPU - never larger, half the bytes on rendered text, a slower encoder, pngLevel 1 only (process-wide once set)
  pngFilter?: 'paeth' | 'adaptive';         // PNG row filters: 'paeth' type 4 on every row (default), 'adaptive' a type per row chosen on the GPU - smaller files, pngLevel 1 only (process-wide once set)
  pngColor?: 'rgba' | 'rgb';                // PNG colour form: 'rgba' colour type 6 (default), 'rgb' colour type 2 - alpha is not read, pngLevel 1 only (process-wide once set; the Canvas shim always exports RGBA)
  devices?: number[];                       // GPUs to shard the stitch over from this process; devices[0] is the root (RCCL gather over xGMI)
  preview?: { width: number; height: number };   // stitchPng / stitchFiles only: also resolve the canvas shrunk to fit this box (the preview node, index.js:1597-1603); refused by stitch, stitchSync, the batches and with `devices`
  split?: 'image' | 'band' | 'rows' | 'auto';   // with devices: image i -> devices[i mod n] | equal output rows per GPU, draw by draw | GPU s owns canvas rows across all draws (horizontal strips: full-width bands) | default 'auto': 'image' when its parts are full-width, else 'rows'
}
export interface PlanRect { image: number; orientation: number; dx: number; dy: number; dw: number; dh: number; }
export interface StitchPlan {
  outW: number; outH: number; scaleDown: number; superSample: number; canvasW: number; canvasH: number;
  bigTask: boolean; rects: PlanRect[];
}
export interface StitchResult { width: number; height: number; data: Buffer; plan: StitchPlan; }
export function stitch(images: StitchImage[], direction: Direction, opts?: StitchOptions): Promise<StitchResult | null>;
export function stitchSync(images: StitchImage[], direction: Direction, opts?: StitchOptions): StitchResult | null;
export function plan(images: StitchImage[], direction: Direction, opts?: StitchOptions): StitchPlan | null;
// one request of a batch: a stitch on the batch's GPU (devices / split / pngLevel / pngColor / pngFilter / pngMatch / preview are refused with a TypeError)
export interface StitchRequest { images: StitchImage[]; direction: Direction; opts?: Omit<StitchOptions, 'devices' | 'split' | 'pngLevel' | 'pngColor' | 'pngFilter' | 'pngMatch' | 'preview' | 'onProgress'>; }
export function stitchBatch(requests: StitchRequest[]): Promise<(StitchResult | null)[]>;
export function stitchBatchSync(requests: StitchRequest[]): (StitchResult | null)[];
export interface Preview { width: number; height: number; data: Buffer; }     // RGBA8, straight alpha, dense rows
export interface StitchPngResult { width: number; height: number; png: Buffer; plan: StitchPlan; preview?: Preview; }   // preview: only when opts.preview was given
export function stitchPng(images: StitchImage[], direction: Direction, opts?: StitchOptions): Promise<StitchPngResult | null>;
export interface PngFormOptions { pngLevel?: 0 | 1; pngColor?: 'rgba' | 'rgb'; pngFilter?: 'paeth' | 'adaptive'; pngMatch?: 'run' | 'window'; }      // one PNG form for a whole call
export function stitchPngBatch(requests: StitchRequest[]): Promise<(StitchPngResult | null)[]>;
export function stitchPngBatchSync(requests: StitchRequest[]): (StitchPngResult | null)[];
export function stitchPngBatch(requests: StitchRequest[], opts: PngFormOptions): Promise<(StitchPngResult | null)[]>;      // one PNG form for the whole batch
export function stitchPngBatchSync(requests: StitchRequest[], opts: PngFormOptions): (StitchPngResult | null)[];
export function encodePng(data: Uint8Array, width: number, height: number, opts?: PngFormOptions): Buffer;
// the export with fileType 'jpg': a baseline JFIF file, pinned byte for byte by include/imagestitch.h (alpha is not read); preview and devices are refused
export interface JpegOptions { quality?: number; subsampling?: '420' | '444' | 420 | 444; optimize?: boolean; }      // quality: an integer 1..100, default 90; subsampling default '420'; optimize default false: the file's own Huffman tables (smaller file, same pixels)
export interface StitchJpegResult { width: number; height: number; jpeg: Buffer; plan: StitchPlan; }
export function stitchJpeg(images: StitchImage[] | Bitmap[], direction: Direction, opts?: Omit<StitchOptions, 'devices' | 'split' | 'preview' | 'pngLevel' | 'pngColor' | 'pngFilter' | 'pngMatch'> & JpegOptions): Promise<StitchJpegResult | null>;
export function encodeJpeg(data: Uint8Array, width: number, height: number, opts?: JpegOptions): Buffer;
// stitchPngBatch with a JPEG in place of each PNG: file k is the file stitchJpeg resolves for request k; null for a request without images
export interface StitchJpegRequest { images: StitchImage[]; direction: Direction; opts?: StitchRequest['opts'] & JpegOptions; }
export function stitchJpegBatch(requests: StitchJpegRequest[]): Promise<(StitchJpegResult | null)[]>;
export function stitchJpegBatchSync(requests: StitchJpegRequest[]): (StitchJpegResult | null)[];
export function setPngLevel(level: 0 | 1): void;
export function setPngColor(color: 'rgba' | 'rgb'): void;
export function setPngFilter(filter: 'paeth' | 'adaptive'): void;
export function setPngMatch(match: 'run' | 'window'): void;
export function decodePng(file: Uint8Array): { width: number; height: number; data: Buffer };
export function stitchFiles(paths: string[], direction: Direction, opts?: StitchOptions, outPath?: string): Promise<StitchPngResult | null>;
export function decodeImage(file: Uint8Array): { width: number; height: number; orientation: number; opaque: boolean; data: Buffer };
// resident bitmaps: images kept in GPU memory; stitch / stitchSync / stitchPng / plan take Bitmap[] in place of StitchImage[] (all or
// none: a mix, or `devices` with bitmaps, is a TypeError; stitchBatch / stitchPngBatch refuse bitmaps)
export class Bitmap {
  private constructor();
  readonly width: number; readonly height: number; readonly orientation: number; readonly opaque: boolean; readonly fileSize: number;
  readonly bmpWidth: number; readonly bmpHeight: number;
  download(): Buffer;       // bmpWidth * bmpHeight * 4 bytes, RGBA8
  preview(width: number, height: number): Preview;   // the stored pixels shrunk to fit the box, reduced in GPU memory (no EXIF turn, as download())
  release(): void;          // idempotent; any other use afterwards throws
}
/** scale: 1, 2, 4 or 8 (one for all files or one per file): a JPEG is decoded at 1 / scale and kept at that size; other types at 1 / 1 */
export function decodeBitmaps(files: (Uint8Array | string)[], opts?: { scale?: 1 | 2 | 4 | 8 | (1 | 2 | 4 | 8)[]; colorProfile?: ColorProfile }): Promise<Bitmap[]>;
// the colour kind of a file's ICC profile: untagged, tagged sRGB, what colorProfile 'srgb' converts, or a profile the contract does not take
export type JoinReason = 'ok' | 'not_jpeg' | 'layout' | 'mixed' | 'tables' | 'size' | 'align' | 'orient' | 'limit' | 'range';
export interface JoinCheck { ok: boolean; reason: JoinReason; image: number; width: number; height: number; subsampling: '444' | '420' | null; }      // image: the first failing image, -1 when ok; width / height: the joined file's, 0 when refused
export function joinJpegCheck(files: (Uint8Array | string)[], direction: Direction): JoinCheck;      // headers only, pure CPU
export function joinJpeg(files: (Uint8Array | string)[], direction: Direction, opts?: { optimize?: boolean }): Promise<Buffer>;      // lossless: the sources' coefficients and tables in one file; rejects for an ineligible set
export function imageColor(file: Uint8Array | string): 'none' | 'identity' | 'convert' | 'unsupported';
/** the largest scale at which a width x height file still decodes to at least minWidth x minHeight pixels (1 if none does) */
export function decodeScaleFit(width: number, height: number, minWidth: number, minHeight: number): 1 | 2 | 4 | 8;
export function uploadBitmap(image: StitchImage): Bitmap;
// the grid of chosen images (index.wxml:4-22): every bitmap as a thumbnail for the cell - 'fill' (default) crops to the cell's aspect ratio
// (aspectFill), 'fit' fits the whole image into it (aspectFit) - turned by its EXIF orientation unless orient is false, all of them
// reduced in GPU memory by one launch pair and brought down in one copy; the results are in the order given
export interface ThumbnailCell { width: number; height: number; mode?: 'fill' | 'fit'; orient?: boolean; }
export function thumbnails(bitmaps: Bitmap[], cell: ThumbnailCell): Promise<Preview[]>;
export function debugBitmapBytes(): number;
export function stitch(images: Bitmap[], direction: Direction, opts?: Omit<StitchOptions, 'devices' | 'split'>): Promise<StitchResult | null>;
export function stitchSync(images: Bitmap[], direction: Direction, opts?: Omit<StitchOptions, 'devices' | 'split'>): StitchResult | null;
export function stitchPng(images: Bitmap[], direction: Direction, opts?: Omit<StitchOptions, 'devices' | 'split'>): Promise<StitchPngResult | null>;
export function plan(images: Bitmap[], direction: Direction, opts?: StitchOptions): StitchPlan | null;
